// The per-sample rules of a VP8 key frame (RFC 6386) and of libwebp's YUV -> BGR tail, as plain functions that csrc/vp8_decode.hip calls from
// its kernels: the 4x4 predictors written per pixel, one row of the inverse DCT, the inverse WHT, the loop filters on a run of samples across an
// edge, the fancy upsampler and the colour conversion.  Free of HIP but for the VP8_HD qualifier, so a host program can call them as well.
// tests/webp_lossy_ref.py restates every one of them.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VP8_HD __host__ __device__ inline
#else
#define VP8_HD inline
#endif

VP8_HD int vp8_clip255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
VP8_HD int vp8_avg2(int a, int b) { return (a + b + 1) >> 1; }
VP8_HD int vp8_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }

// One pixel (x, y) of a 4x4 prediction.  e[0 .. 12] = L K J I | X | A B C D E F G H: the left column bottom to top, the corner, the row above
// and above-right (the edge array of the RFC); with B = e + 4, B[0] is the corner, B[k] the k-th sample above, B[-k] the k-th sample to the left.
VP8_HD int vp8_pred4(int mode, const int* e, int x, int y) {
    const int* B = e + 4;
    const int* T = e + 5;                          // the 8 samples above
    switch (mode) {
        case 0: return (T[0] + T[1] + T[2] + T[3] + e[0] + e[1] + e[2] + e[3] + 4) >> 3;                                  // DC
        case 1: return vp8_clip255(T[x] + B[-1 - y] - B[0]);                                                              // TM
        case 2: return vp8_avg3(B[x], B[x + 1], B[x + 2]);                                                                // VE
        case 3: return vp8_avg3(B[-y], B[-1 - y], B[y == 3 ? -4 : -2 - y]);                                               // HE
        case 4: { const int d = x - y; return vp8_avg3(B[d - 1], B[d], B[d + 1]); }                                       // RD
        case 5: {                                                                                                         // VR
            if (x >= 1 && y >= 2) { x -= 1; y -= 2; }
            if (y == 0) return vp8_avg2(B[x], B[x + 1]);
            if (y == 1) return vp8_avg3(B[x - 1], B[x], B[x + 1]);
            return y == 2 ? vp8_avg3(B[-2], B[-1], B[0]) : vp8_avg3(B[-3], B[-2], B[-1]);                                 // x == 0
        }
        case 6: { const int i = x + y; return vp8_avg3(T[i], T[i + 1], T[i == 6 ? 7 : i + 2]); }                          // LD
        case 7: {                                                                                                         // VL
            if (x == 3 && y >= 2) return y == 2 ? vp8_avg3(T[4], T[5], T[6]) : vp8_avg3(T[5], T[6], T[7]);
            const int i = x + (y >> 1);
            return (y & 1) ? vp8_avg3(T[i], T[i + 1], T[i + 2]) : vp8_avg2(T[i], T[i + 1]);
        }
        case 8: {                                                                                                         // HD
            while (x >= 2 && y >= 1) { x -= 2; y -= 1; }
            if (x == 0) return vp8_avg2(B[-y - 1], B[-y]);
            if (x == 1) return vp8_avg3(B[-y - 1], B[-y], B[-y + 1]);
            return vp8_avg3(B[x - 2], B[x - 1], B[x]);                                                                    // y == 0, x = 2 or 3
        }
        default: {                                                                                                        // HU
            const int i = 2 * y + x;                   // l(k) = B[-1 - k]
            if (i >= 6) return B[-4];
            const int k = i >> 1;
            return (i & 1) ? vp8_avg3(B[-1 - k], B[-2 - k], B[k == 2 ? -4 : -3 - k]) : vp8_avg2(B[-1 - k], B[-2 - k]);
        }
    }
}

VP8_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
VP8_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }

// Row i of the 4 x 4 residual of 16 coefficients in raster order (both passes of the inverse DCT) -> r[0 .. 3]
template <typename T>
VP8_HD void vp8_idct_row(const T* c, int i, int* r) {
    int t[4];
    for (int j = 0; j < 4; ++j) {                  // first pass on column j, element i of its four results
        const int c0 = c[j], c1 = c[4 + j], c2 = c[8 + j], c3 = c[12 + j];
        const int a = c0 + c2, b = c0 - c2;
        const int cc = vp8_mul2(c1) - vp8_mul1(c3), dd = vp8_mul1(c1) + vp8_mul2(c3);
        t[j] = i == 0 ? a + dd : i == 1 ? b + cc : i == 2 ? b - cc : a - dd;
    }
    const int dc = t[0] + 4;
    const int a = dc + t[2], b = dc - t[2];
    const int cc = vp8_mul2(t[1]) - vp8_mul1(t[3]), dd = vp8_mul1(t[1]) + vp8_mul2(t[3]);
    r[0] = (a + dd) >> 3; r[1] = (b + cc) >> 3; r[2] = (b - cc) >> 3; r[3] = (a - dd) >> 3;
}

// Output `o` (0 .. 15: the DC of luma block o) of the inverse WHT of the 16 Y2 coefficients in raster order
template <typename T>
VP8_HD int vp8_iwht(const T* c, int o) {
    const int i = o >> 2, k = o & 3;
    int t[4];
    for (int j = 0; j < 4; ++j) {
        const int a0 = c[j] + c[12 + j], a1 = c[4 + j] + c[8 + j], a2 = c[4 + j] - c[8 + j], a3 = c[j] - c[12 + j];
        t[j] = i == 0 ? a0 + a1 : i == 1 ? a3 + a2 : i == 2 ? a0 - a1 : a3 - a2;
    }
    const int dc = t[0] + 3;
    const int a0 = dc + t[3], a1 = t[1] + t[2], a2 = t[1] - t[2], a3 = dc - t[3];
    return (k == 0 ? a0 + a1 : k == 1 ? a3 + a2 : k == 2 ? a0 - a1 : a3 - a2) >> 3;
}

// ---- loop filters on the 8 samples s[0 .. 7] = p3 p2 p1 p0 | q0 q1 q2 q3 across an edge
VP8_HD int vp8_abs(int v) { return v < 0 ? -v : v; }
VP8_HD int vp8_sclip1(int v) { return v < -128 ? -128 : v > 127 ? 127 : v; }
VP8_HD int vp8_sclip2(int v) { return v < -16 ? -16 : v > 15 ? 15 : v; }

VP8_HD void vp8_filter2(int* s) {
    const int a = 3 * (s[4] - s[3]) + vp8_sclip1(s[2] - s[5]);
    const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3);
    s[3] = vp8_clip255(s[3] + a2);
    s[4] = vp8_clip255(s[4] - a1);
}
VP8_HD void vp8_filter4(int* s) {
    const int a = 3 * (s[4] - s[3]);
    const int a1 = vp8_sclip2((a + 4) >> 3), a2 = vp8_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
    s[2] = vp8_clip255(s[2] + a3);
    s[3] = vp8_clip255(s[3] + a2);
    s[4] = vp8_clip255(s[4] - a1);
    s[5] = vp8_clip255(s[5] - a3);
}
VP8_HD void vp8_filter6(int* s) {
    const int a = vp8_sclip1(3 * (s[4] - s[3]) + vp8_sclip1(s[2] - s[5]));
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    s[1] = vp8_clip255(s[1] + a3);
    s[2] = vp8_clip255(s[2] + a2);
    s[3] = vp8_clip255(s[3] + a1);
    s[4] = vp8_clip255(s[4] - a1);
    s[5] = vp8_clip255(s[5] - a2);
    s[6] = vp8_clip255(s[6] - a3);
}
// the simple filter (luma only): thresh = limit + 4 on a macroblock edge, limit on an inner edge
VP8_HD void vp8_simple_filter(int* s, int thresh) {
    if (4 * vp8_abs(s[3] - s[4]) + vp8_abs(s[2] - s[5]) <= 2 * thresh + 1) vp8_filter2(s);
}
// the normal filter; mb_edge: a macroblock edge (6 samples change) or an inner edge (4 samples)
VP8_HD void vp8_normal_filter(int* s, int thresh, int ithresh, int hev_thresh, bool mb_edge) {
    if (4 * vp8_abs(s[3] - s[4]) + vp8_abs(s[2] - s[5]) > 2 * thresh + 1) return;
    if (vp8_abs(s[0] - s[1]) > ithresh || vp8_abs(s[1] - s[2]) > ithresh || vp8_abs(s[2] - s[3]) > ithresh || vp8_abs(s[7] - s[6]) > ithresh ||
        vp8_abs(s[6] - s[5]) > ithresh || vp8_abs(s[5] - s[4]) > ithresh)
        return;
    if (vp8_abs(s[2] - s[3]) > hev_thresh || vp8_abs(s[5] - s[4]) > hev_thresh) vp8_filter2(s);
    else if (mb_edge) vp8_filter6(s);
    else vp8_filter4(s);
}

// ---- libwebp's fancy upsampler: N the nearest chroma sample, H / V its horizontal / vertical neighbour, D the diagonal one (two roundings)
VP8_HD int vp8_upsample(int N, int H, int V, int D) { return (((N + H + V + D + 8 + 2 * (H + V)) >> 3) + N) >> 1; }
// the nearest chroma index of output index i and the neighbour on its other side, clamped into 0 .. n - 1
VP8_HD void vp8_chroma_pair(int i, int n, int* nearest, int* other) {
    const int a = (i & 1) ? (i - 1) >> 1 : i >> 1;
    const int b = (i & 1) ? a + 1 : a - 1;
    *nearest = a;
    *other = b < 0 ? 0 : b > n - 1 ? n - 1 : b;
}
// libwebp's 14-bit fixed point YUV -> BGR
VP8_HD int vp8_clip6(int v) { return (v & ~16383) == 0 ? v >> 6 : v < 0 ? 0 : 255; }
VP8_HD void vp8_yuv_to_bgr(int y, int u, int v, uint8_t* bgr) {
    const int yy = (y * 19077) >> 8;
    bgr[0] = (uint8_t)vp8_clip6(yy + ((u * 33050) >> 8) - 17685);
    bgr[1] = (uint8_t)vp8_clip6(yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708);
    bgr[2] = (uint8_t)vp8_clip6(yy + ((v * 26149) >> 8) - 14234);
}
