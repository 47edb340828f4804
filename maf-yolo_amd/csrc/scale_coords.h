// Evaler.scale_coords with ratio_pad (yolov6/core/evaler.py:382-409) on one xyxy box, shared by post.hip and pr_metric.hip.
// par = the maf_coco_rows image parameters: h0, w0, gain applied to x, gain applied to y, pad_w, pad_h (fp32).  Subtract the pad,
// IEEE-divide by the gain, clamp to [0, w0] / [0, h0]: the reference's fp32 tensor ops in their order.  Compile the including file
// with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void maf_scale_box(float& x1, float& y1, float& x2, float& y2, const float* par) {
    const float h0 = par[0], w0 = par[1], gx = par[2], gy = par[3], pw = par[4], ph = par[5];
    x1 = (x1 - pw) / gx; y1 = (y1 - ph) / gy; x2 = (x2 - pw) / gx; y2 = (y2 - ph) / gy;
    x1 = fminf(fmaxf(x1, 0.f), w0); x2 = fminf(fmaxf(x2, 0.f), w0);
    y1 = fminf(fmaxf(y1, 0.f), h0); y2 = fminf(fmaxf(y2, 0.f), h0);
}
