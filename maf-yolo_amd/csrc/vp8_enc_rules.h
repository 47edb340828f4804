// The per-sample rules of the VP8 ENCODER (csrc/vp8_encode.hip) as plain functions: BGR -> Y, U, V, the forward 4x4 DCT and WHT (the integer
// forms of libwebp's FTransform / FTransformWHT) and the quantiser.  Free of HIP but for the VP8_HD qualifier of vp8_rules.h, so a host
// program can call them as well (tests/test_webp_lossy_encode_host.py builds one).  tests/webp_lossy_encode_ref.py restates every one of them.
#pragma once
#include "vp8_rules.h"

// integer BT.601; the chroma formulas take the plain SUM of a 2x2 block (no gamma-aware averaging: this project's rule, not libwebp's converter)
VP8_HD int vp8e_luma(int r, int g, int b) { return (16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16; }
VP8_HD int vp8e_chroma_u(int r4, int g4, int b4) { return (-9719 * r4 - 19081 * g4 + 28800 * b4 + (128 << 18) + (1 << 17)) >> 18; }
VP8_HD int vp8e_chroma_v(int r4, int g4, int b4) { return (28800 * r4 - 24116 * g4 - 4684 * b4 + (128 << 18) + (1 << 17)) >> 18; }

// the 4 x 4 residual d (raster order) -> 16 coefficients in raster order
VP8_HD void vp8e_fdct(const int* d, int* out) {
    int tmp[16];
    for (int i = 0; i < 4; ++i) {
        const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
        tmp[4 * i] = (a0 + a1) * 8;
        tmp[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
        tmp[4 * i + 2] = (a0 - a1) * 8;
        tmp[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
    }
    for (int i = 0; i < 4; ++i) {
        const int a0 = tmp[i] + tmp[12 + i], a1 = tmp[4 + i] + tmp[8 + i], a2 = tmp[4 + i] - tmp[8 + i], a3 = tmp[i] - tmp[12 + i];
        out[i] = (a0 + a1 + 7) >> 4;
        out[4 + i] = ((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0);
        out[8 + i] = (a0 - a1 + 7) >> 4;
        out[12 + i] = (a3 * 2217 - a2 * 5352 + 51000) >> 16;
    }
}

// Output `o` (raster order) of the forward WHT of the DC of the 16 luma blocks
template <typename T>
VP8_HD int vp8e_fwht(const T* dc, int o) {
    const int k = o >> 2, i = o & 3;                 // second-pass output k of column i
    int t[4];
    for (int j = 0; j < 4; ++j) {                    // first pass on row j, its element i
        const int a0 = dc[4 * j] + dc[4 * j + 2], a1 = dc[4 * j + 1] + dc[4 * j + 3], a2 = dc[4 * j + 1] - dc[4 * j + 3], a3 = dc[4 * j] - dc[4 * j + 2];
        t[j] = i == 0 ? a0 + a1 : i == 1 ? a3 + a2 : i == 2 ? a3 - a2 : a0 - a1;
    }
    const int a0 = t[0] + t[2], a1 = t[1] + t[3], a2 = t[1] - t[3], a3 = t[0] - t[2];
    return (k == 0 ? a0 + a1 : k == 1 ? a3 + a2 : k == 2 ? a3 - a2 : a0 - a1) >> 1;
}

// level = sign(c) * min((|c| + (q >> 1)) / q, 2047)
VP8_HD int vp8e_quantise(int c, int q) {
    int a = ((c < 0 ? -c : c) + (q >> 1)) / q;
    if (a > 2047) a = 2047;
    return c < 0 ? -a : a;
}

// One sample (x, y) of a 16x16 or 8x8 prediction (n = 16, 8) of mode DC, TM, V, H = 0 .. 3.  e: the corner, the n samples above, the n samples
// to the left (with the format's 127 / 129 borders already in place); dc: the DC value of the block.
VP8_HD int vp8e_pred(int mode, const uint8_t* e, int n, int x, int y, int dc) {
    return mode == 0 ? dc : mode == 1 ? vp8_clip255(e[1 + x] + e[1 + n + y] - e[0]) : mode == 2 ? e[1 + x] : e[1 + n + y];
}
// the DC value: the mean of the neighbours that exist, 128 without any
VP8_HD int vp8e_dc(const uint8_t* e, int n, bool has_left, bool has_top) {
    int top = 0, left = 0;
    for (int i = 0; i < n; ++i) { top += e[1 + i]; left += e[1 + n + i]; }
    const int sh = n == 16 ? 4 : 3;
    return has_left && has_top ? (top + left + n) >> (sh + 1) : has_top ? (top + (n >> 1)) >> sh : has_left ? (left + (n >> 1)) >> sh : 128;
}
