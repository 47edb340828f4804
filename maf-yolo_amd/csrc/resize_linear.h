// OpenCV's uint8 INTER_LINEAR coefficient rule (imgproc/resize.cpp), shared by letterbox.hip and augment.hip; restated in
// tests/letterbox_ref.py.  Compile the including file with -ffp-contract=off: the double -> float sequence must not fuse.
#pragma once
#include <hip/hip_runtime.h>

// OpenCV's coefficient sequence for one destination index (resize.cpp: float(... in double ...), cvFloor, fx -= sx)
__device__ __forceinline__ void lin_coef(int d, double scale, int& s, float& f) {
    f = (float)(((double)d + 0.5) * scale - 0.5);
    s = (int)floorf(f);
    f -= (float)s;
}
__device__ __forceinline__ int coef_q(float c) { return (int)rintf(c * 2048.f); }
