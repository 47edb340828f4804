// Training augmentation on the device: load_image's resize, then mosaic + random_affine + mixup + augment_hsv + flips + HWC -> CHW / BGR -> RGB
// in one launch per batch (the pixel work of TrainValDataset.__getitem__, yolov6/data/datasets.py:147-275).
//
// Pixel rules: tests/augment_ref.py (its docstring lists every rule); the kernels equal that restatement bit for bit.
//   resize:   OpenCV's uint8 INTER_LINEAR as in letterbox.hip (resize_linear.h), the exact-2x area-fast average, a copy for equal sizes
//   warp:     warpAffine's fixed point: adelta = rint(m0 x 1024), X0 = rint((m1 y + m2) 1024) + 16 (double), X = (X0 + adelta) >> 5,
//             sx = X >> 5 (int16-saturated), fx = X & 31; weights (32 - fx)(32 - fy) 32, ... (sum 32768); (sum + (1 << 14)) >> 15;
//             every neighbour outside the tiles is 114 (the canvas fill and BORDER_CONSTANT alike)
//   mixup:    (a r + b (1 - r)) in double, truncated
//   HSV:      uint8 BGR2HSV (hsv_shift 12, sdiv / hdiv tables, hue range 180), the three tables, uint8 HSV2BGR in float
//
// Shapes.  augment_resize_kernel: grid (bands of RS_ROWS output rows, frames), one output pixel per lane and step, plain byte loads (the
// reads of one row band are a few contiguous source rows).  mosaic_affine_kernel: grid (bands of MA_ROWS output rows, B); a workgroup
// builds the HSV division tables and copies its sample's three tables into LDS, then each lane computes 4 adjacent output pixels of a row
// (the flips are an index map: output (x, y) is pre-flip pixel (x or S-1-x, y or S-1-y)) and writes them as one 32-bit store per plane.
// The canvas is never materialised: each of the 4 taps of a pixel is looked up in the <= 4 tile rectangles of its layer (sample
// parameters are workgroup-uniform: scalar loads).  Every output byte is written exactly once; every frame read is inside the frame
// (the host checks each tile's rectangle + offset against the frame before the launch).
//
// copy_paste (maf_mosaic_affine_paste, PASTE = true in the shared device code): a layer may carry the bit mask maf_polygon_mask
// (polygon_mask.hip) drew for its pasted contours; a tap at canvas (x, y) inside [0, C)^2 then reads canvas (C-1-x, y) where bit (C-1-x, y)
// is set: im[flip(im_new) != 0] = flip(im)[...] of data_augment.py:303-305 without a second canvas.  One 32-bit mask load per tap, from
// the C^2 / 8 bytes of the layer's mask.
#include "maf_common.h"
#include "resize_linear.h"

namespace {

constexpr int RS_ROWS = 4;                 // resize: output rows per workgroup
constexpr int MA_ROWS = 8;                 // mosaic_affine: output rows per workgroup (S is a multiple of 32)
constexpr int THREADS = 256;
constexpr int GREY = 114;

__global__ __launch_bounds__(THREADS) void augment_resize_kernel(const maf_augment_frame_t* __restrict__ frames) {
    const maf_augment_frame_t f = frames[blockIdx.y];
    const int y0 = blockIdx.x * RS_ROWS;
    if (y0 >= f.new_h) return;                                  // the grid covers the tallest frame
    const int y1 = min(y0 + RS_ROWS, f.new_h);
    const int w = f.w, h = f.h, nw = f.new_w, nh = f.new_h;
    const bool copy = (w == nw && h == nh), area2 = (w == 2 * nw && h == 2 * nh);
    const double scx = 1.0 / ((double)nw / (double)w), scy = 1.0 / ((double)nh / (double)h);
    const int n = (y1 - y0) * nw;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int yy = i / nw, x = i - yy * nw, y = y0 + yy;
        uint8_t* d = f.dst + ((size_t)y * nw + x) * 3;
        if (copy) {
            const uint8_t* s = f.src + (size_t)y * f.src_pitch + 3 * x;
            d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
        } else if (area2) {
            const uint8_t* s0 = f.src + (size_t)(2 * y) * f.src_pitch + 6 * x;
            const uint8_t* s1 = s0 + f.src_pitch;
            for (int c = 0; c < 3; ++c) d[c] = (uint8_t)(((int)s0[c] + s0[c + 3] + s1[c] + s1[c + 3] + 2) >> 2);
        } else {
            int sx, sy;
            float fx, fy;
            lin_coef(x, scx, sx, fx);
            if (sx < 0) { sx = 0; fx = 0.f; }
            if (sx >= w - 1) { sx = w - 1; fx = 0.f; }
            const int a0 = coef_q(1.f - fx), a1 = coef_q(fx);
            lin_coef(y, scy, sy, fy);                           // rows: no coefficient clamp, only the index is clamped
            const int b0 = coef_q(1.f - fy), b1 = coef_q(fy);
            const int r0 = sy < 0 ? 0 : (sy >= h ? h - 1 : sy), r1 = sy + 1 < 0 ? 0 : (sy + 1 >= h ? h - 1 : sy + 1);
            const uint8_t* p0 = f.src + (size_t)r0 * f.src_pitch + 3 * sx;
            const uint8_t* p1 = f.src + (size_t)r1 * f.src_pitch + 3 * sx;
            const int o1 = a1 ? 3 : 0;                          // a1 = 0 at a clamped column: never read past the row
            for (int c = 0; c < 3; ++c) {
                const int S0 = p0[c] * a0 + p0[c + o1] * a1, S1 = p1[c] * a0 + p1[c + o1] * a1;
                const int t = ((((S0 >> 4) * b0) >> 16) + (((S1 >> 4) * b1) >> 16) + 2) >> 2;
                d[c] = (uint8_t)(t < 0 ? 0 : (t > 255 ? 255 : t));
            }
        }
    }
}

// canvas pixel (cx, cy) of a layer: the tile whose rectangle holds it, else 114
__device__ __forceinline__ void canvas_px(const maf_augment_tile_t* __restrict__ t, int nt, int cx, int cy, int& b, int& g, int& r) {
    for (int k = 0; k < nt; ++k) {
        if (cx >= t[k].x0 && cx < t[k].x1 && cy >= t[k].y0 && cy < t[k].y1) {
            const uint8_t* p = t[k].ptr + (size_t)(cy + t[k].dy) * t[k].pitch + 3 * (cx + t[k].dx);
            b = p[0]; g = p[1]; r = p[2];
            return;
        }
    }
    b = g = r = GREY;
}

// canvas_px after copy_paste: inside [0, C)^2 the mirrored pixel where the mask is set there; outside, 114
__device__ __forceinline__ void pasted_px(const maf_augment_tile_t* __restrict__ t, int nt, const uint32_t* __restrict__ mask, int C, int cx, int cy,
                                          int& b, int& g, int& r) {
    if ((unsigned)cx >= (unsigned)C || (unsigned)cy >= (unsigned)C) {
        b = g = r = GREY;
        return;
    }
    const int mx = C - 1 - cx;
    if ((mask[(size_t)cy * (C >> 5) + (mx >> 5)] >> (mx & 31)) & 1u) cx = mx;
    canvas_px(t, nt, cx, cy, b, g, r);
}

// warpAffine INTER_LINEAR of one layer at output pixel (px, py) -> BGR; PASTE: the layer's copy_paste mask (may be null) over a C x C canvas
template <bool PASTE>
__device__ __forceinline__ void warp_px(const double* __restrict__ m, const maf_augment_tile_t* __restrict__ t, int nt, const uint32_t* __restrict__ mask,
                                        int C, int px, int py, int* bgr) {
    const int X = ((int)rint((m[1] * py + m[2]) * 1024.0) + 16 + (int)rint(m[0] * px * 1024.0)) >> 5;
    const int Y = ((int)rint((m[4] * py + m[5]) * 1024.0) + 16 + (int)rint(m[3] * px * 1024.0)) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);
    const int fx = X & 31, fy = Y & 31;
    const int w0 = (32 - fx) * (32 - fy) * 32, w1 = fx * (32 - fy) * 32, w2 = (32 - fx) * fy * 32, w3 = fx * fy * 32;
    int v[4][3];
    if (PASTE && mask) {                                        // workgroup-uniform
        pasted_px(t, nt, mask, C, sx, sy, v[0][0], v[0][1], v[0][2]);
        pasted_px(t, nt, mask, C, sx + 1, sy, v[1][0], v[1][1], v[1][2]);
        pasted_px(t, nt, mask, C, sx, sy + 1, v[2][0], v[2][1], v[2][2]);
        pasted_px(t, nt, mask, C, sx + 1, sy + 1, v[3][0], v[3][1], v[3][2]);
    } else {
        canvas_px(t, nt, sx, sy, v[0][0], v[0][1], v[0][2]);
        canvas_px(t, nt, sx + 1, sy, v[1][0], v[1][1], v[1][2]);
        canvas_px(t, nt, sx, sy + 1, v[2][0], v[2][1], v[2][2]);
        canvas_px(t, nt, sx + 1, sy + 1, v[3][0], v[3][1], v[3][2]);
    }
    for (int c = 0; c < 3; ++c) bgr[c] = (v[0][c] * w0 + v[1][c] * w1 + v[2][c] * w2 + v[3][c] * w3 + (1 << 14)) >> 15;
}

__device__ __forceinline__ int round_u8(float x) {
    const int v = (int)rintf(x);
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// uint8 BGR2HSV -> tables -> uint8 HSV2BGR, in place on bgr
__device__ __forceinline__ void hsv_px(int* bgr, const int* sdiv, const int* hdiv, const uint8_t* lut) {
    const int b = bgr[0], g = bgr[1], r = bgr[2];
    int v = max(b, max(g, r));
    const int diff = v - min(b, min(g, r));
    int s = (diff * sdiv[v] + (1 << 11)) >> 12;
    int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
    h = (h * hdiv[diff] + (1 << 11)) >> 12;
    if (h < 0) h += 180;
    h = lut[h]; s = lut[256 + s]; v = lut[512 + v];
    const float sf = (float)s * (1.0f / 255.0f), vf = (float)v;
    if (sf == 0.f) {
        bgr[0] = bgr[1] = bgr[2] = round_u8(vf);
        return;
    }
    float hf = fmodf((float)h * (6.0f / 180.0f), 6.0f);
    int sector = (int)floorf(hf);
    hf -= (float)sector;
    if ((unsigned)sector >= 6u) { sector = 0; hf = 0.f; }
    const float t0 = vf, t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * hf), t3 = vf * (1.f - sf * (1.f - hf));
    float ob, og, orr;
    switch (sector) {                                           // OpenCV's sector_data {1,3,0} {1,0,2} {3,0,1} {0,2,1} {0,1,3} {2,1,0}
        case 0: ob = t1; og = t3; orr = t0; break;
        case 1: ob = t1; og = t0; orr = t2; break;
        case 2: ob = t3; og = t0; orr = t1; break;
        case 3: ob = t0; og = t2; orr = t1; break;
        case 4: ob = t0; og = t1; orr = t3; break;
        default: ob = t2; og = t1; orr = t0; break;
    }
    bgr[0] = round_u8(ob); bgr[1] = round_u8(og); bgr[2] = round_u8(orr);
}

template <bool PASTE>
__device__ __forceinline__ void mosaic_affine_body(const maf_augment_sample_t* __restrict__ samples, const maf_augment_paste_t* __restrict__ paste, int S,
                                                   uint8_t* __restrict__ out) {
    __shared__ int sdiv[256], hdiv[256];
    __shared__ uint8_t lut[768];
    const int b = blockIdx.y;
    const maf_augment_sample_t* sm = samples + b;
    const int hsv = sm->hsv;
    if (hsv) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) {
            sdiv[i] = i ? (int)rint((double)(255 << 12) / (1.0 * i)) : 0;
            hdiv[i] = i ? (int)rint((double)(180 << 12) / (6.0 * i)) : 0;
        }
        for (int i = threadIdx.x; i < 768; i += blockDim.x) lut[i] = (&sm->lut[0][0])[i];
    }
    __syncthreads();
    const int nt0 = sm->ntiles[0], nt1 = sm->ntiles[1];
    const uint32_t* mask0 = PASTE ? paste[b].mask[0] : nullptr;
    const uint32_t* mask1 = PASTE ? paste[b].mask[1] : nullptr;
    const int C = PASTE ? paste[b].C : 0;
    const int flipud = sm->flipud, fliplr = sm->fliplr;
    const double r = sm->r, r1 = 1.0 - r;
    const int nq = S >> 2;
    const size_t plane = (size_t)S * S;
    uint8_t* o = out + (size_t)b * 3 * plane;
    for (int q = threadIdx.x; q < MA_ROWS * nq; q += blockDim.x) {
        const int y = blockIdx.x * MA_ROWS + q / nq, x4 = (q % nq) * 4;
        const int py = flipud ? S - 1 - y : y;
        uint32_t word[3] = {0u, 0u, 0u};
        for (int j = 0; j < 4; ++j) {
            const int px = fliplr ? S - 1 - (x4 + j) : x4 + j;
            int bgr[3];
            warp_px<PASTE>(sm->minv[0], sm->tile[0], nt0, mask0, C, px, py, bgr);
            if (nt1) {
                int o2[3];
                warp_px<PASTE>(sm->minv[1], sm->tile[1], nt1, mask1, C, px, py, o2);
                for (int c = 0; c < 3; ++c) bgr[c] = (int)((double)bgr[c] * r + (double)o2[c] * r1);
            }
            if (hsv) hsv_px(bgr, sdiv, hdiv, lut);
            for (int p = 0; p < 3; ++p) word[p] |= (uint32_t)bgr[2 - p] << (8 * j);     // plane p = R, G, B
        }
        for (int p = 0; p < 3; ++p) reinterpret_cast<uint32_t*>(o + p * plane + (size_t)y * S)[x4 >> 2] = word[p];
    }
}

__global__ __launch_bounds__(THREADS) void mosaic_affine_kernel(const maf_augment_sample_t* __restrict__ samples, int S, uint8_t* __restrict__ out) {
    mosaic_affine_body<false>(samples, nullptr, S, out);
}

__global__ __launch_bounds__(THREADS) void mosaic_affine_paste_kernel(const maf_augment_sample_t* __restrict__ samples,
                                                                      const maf_augment_paste_t* __restrict__ paste, int S, uint8_t* __restrict__ out) {
    mosaic_affine_body<true>(samples, paste, S, out);
}

}  // namespace

extern "C" int32_t maf_augment_paste_size(void) { return (int32_t)sizeof(maf_augment_paste_t); }
extern "C" int32_t maf_augment_sample_size(void) { return (int32_t)sizeof(maf_augment_sample_t); }

extern "C" int maf_augment_resize(const maf_augment_frame_t* frames, const maf_augment_frame_t* frames_dev, int32_t n, maf_stream_t stream) {
    MAF_REQUIRE(frames && frames_dev, "augment_resize: null pointer (host table and its device copy)");
    MAF_REQUIRE(n > 0, "augment_resize: n must be positive");
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        const maf_augment_frame_t& f = frames[i];
        MAF_REQUIRE(f.src && f.dst, "augment_resize: null frame pointer");
        MAF_REQUIRE(f.h > 0 && f.w > 0 && f.new_h > 0 && f.new_w > 0, "augment_resize: sizes must be positive");
        MAF_REQUIRE(f.src_pitch >= 3 * (int64_t)f.w, "augment_resize: the source row pitch must be at least 3 w bytes");
        MAF_REQUIRE((int64_t)f.new_w * f.new_h < (int64_t)1 << 28 && (int64_t)f.h * f.src_pitch < (int64_t)1 << 40, "augment_resize: frame too large");
        max_h = f.new_h > max_h ? f.new_h : max_h;
    }
    hipLaunchKernelGGL(augment_resize_kernel, dim3((max_h + RS_ROWS - 1) / RS_ROWS, n), dim3(THREADS), 0, static_cast<hipStream_t>(stream), frames_dev);
    return maf_check_hip(hipGetLastError(), "augment_resize launch");
}

// the checks of maf_mosaic_affine's arguments, shared with maf_mosaic_affine_paste
static int check_mosaic_affine(const maf_augment_sample_t* samples, const maf_augment_sample_t* samples_dev, int32_t B, int32_t S, uint8_t* out) {
    MAF_REQUIRE(samples && samples_dev && out, "mosaic_affine: null pointer (host table, its device copy, out)");
    MAF_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "mosaic_affine: out must be 4-byte aligned (32-bit stores)");
    MAF_REQUIRE(B > 0, "mosaic_affine: B must be positive");
    MAF_REQUIRE(S > 0 && S % 32 == 0 && S <= 8192, "mosaic_affine: S must be a positive multiple of 32 (at most 8192)");
    for (int i = 0; i < B; ++i) {
        const maf_augment_sample_t& s = samples[i];
        MAF_REQUIRE(s.ntiles[0] >= 1 && s.ntiles[0] <= MAF_AUGMENT_MAX_TILES && s.ntiles[1] >= 0 && s.ntiles[1] <= MAF_AUGMENT_MAX_TILES,
                    "mosaic_affine: layer 0 needs 1..4 tiles, layer 1 (mixup) 0..4");
        MAF_REQUIRE((s.hsv | s.flipud | s.fliplr) >= 0 && s.hsv <= 1 && s.flipud <= 1 && s.fliplr <= 1, "mosaic_affine: hsv / flipud / fliplr are 0 or 1");
        for (int l = 0; l < 2; ++l)
            for (int k = 0; k < s.ntiles[l]; ++k) {
                const maf_augment_tile_t& t = s.tile[l][k];
                MAF_REQUIRE(t.ptr && t.h > 0 && t.w > 0 && t.pitch >= 3 * (int64_t)t.w, "mosaic_affine: a tile needs a frame (pointer, h, w > 0, pitch >= 3 w)");
                MAF_REQUIRE(t.x0 <= t.x1 && t.y0 <= t.y1 && t.x0 > -(1 << 20) && t.y0 > -(1 << 20) && t.x1 < (1 << 20) && t.y1 < (1 << 20),
                            "mosaic_affine: bad tile rectangle");
                MAF_REQUIRE(t.x0 == t.x1 || t.y0 == t.y1 ||
                            ((int64_t)t.x0 + t.dx >= 0 && (int64_t)t.x1 + t.dx <= t.w && (int64_t)t.y0 + t.dy >= 0 && (int64_t)t.y1 + t.dy <= t.h),
                            "mosaic_affine: a tile rectangle reads outside its frame");
            }
    }
    return 0;
}

extern "C" int maf_mosaic_affine(const maf_augment_sample_t* samples, const maf_augment_sample_t* samples_dev, int32_t B, int32_t S, uint8_t* out,
                                 maf_stream_t stream) {
    if (int rc = check_mosaic_affine(samples, samples_dev, B, S, out)) return rc;
    hipLaunchKernelGGL(mosaic_affine_kernel, dim3(S / MA_ROWS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), samples_dev, (int)S, out);
    return maf_check_hip(hipGetLastError(), "mosaic_affine launch");
}

extern "C" int maf_mosaic_affine_paste(const maf_augment_sample_t* samples, const maf_augment_sample_t* samples_dev, const maf_augment_paste_t* paste,
                                       const maf_augment_paste_t* paste_dev, int32_t B, int32_t S, uint8_t* out, maf_stream_t stream) {
    MAF_REQUIRE(paste && paste_dev, "mosaic_affine_paste: null pointer (host paste table, its device copy)");
    if (int rc = check_mosaic_affine(samples, samples_dev, B, S, out)) return rc;
    MAF_REQUIRE((reinterpret_cast<uintptr_t>(paste_dev) & 7) == 0, "mosaic_affine_paste: paste_dev must be 8-byte aligned");
    for (int i = 0; i < B; ++i) {
        const maf_augment_paste_t& p = paste[i];
        MAF_REQUIRE(p.C == 2 * S, "mosaic_affine_paste: the canvas side C must be 2 S");
        for (int l = 0; l < 2; ++l) {
            if (!p.mask[l]) continue;
            MAF_REQUIRE((reinterpret_cast<uintptr_t>(p.mask[l]) & 3) == 0, "mosaic_affine_paste: a mask must be 4-byte aligned");
            MAF_REQUIRE(samples[i].ntiles[l] > 0, "mosaic_affine_paste: a mask for a layer without tiles");
            for (int k = 0; k < samples[i].ntiles[l]; ++k) {
                const maf_augment_tile_t& t = samples[i].tile[l][k];
                MAF_REQUIRE(t.x0 >= 0 && t.y0 >= 0 && t.x1 <= p.C && t.y1 <= p.C, "mosaic_affine_paste: a tile of a pasted layer leaves the C x C canvas");
            }
        }
    }
    hipLaunchKernelGGL(mosaic_affine_paste_kernel, dim3(S / MA_ROWS, B), dim3(THREADS), 0, static_cast<hipStream_t>(stream), samples_dev, paste_dev,
                       (int)S, out);
    return maf_check_hip(hipGetLastError(), "mosaic_affine_paste launch");
}
