// Lossy WebP (one VP8 key frame, RFC 6386) encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any
// row pitch), RIFF / WEBP files out that libwebp and csrc/vp8_decode.hip decode to the same frame.  Replaces cv2.imwrite(path, img,
// [cv2.IMWRITE_WEBP_QUALITY, q]) for the crops and annotated frames a detector leaves behind.  What is written is restated rule by rule in
// tests/webp_lossy_encode_ref.py, whose bytes the device equals; the per-sample arithmetic is in vp8_enc_rules.h and vp8_rules.h, the
// constants of the format in vp8_tables.h; the host side (sizes, the job table) is maf-yolo_amd/webp_lossy_encode.py;
// include/mafyolo_vp8_encode.h lists the kernels, the blob and the buffers.
//
// Bounded by construction: every loop bound is a host-validated count (macroblocks, 25 blocks, 16 coefficients, 11 extra bits, at most 8
// partitions); every store of the bool coder is compared with its partition's capacity (sized from MAF_VP8_ENC_PART_BOUND), every store into
// the output with out_bytes.
#include "maf_common.h"
#include "../../include/mafyolo_vp8_encode.h"
#include "image_blob.h"
#include "block_scan.h"
#include "vp8_enc_rules.h"

namespace {

#include "vp8_tables.h"        // inside the namespace: csrc/vp8_decode.hip holds the same tables under the same names

constexpr int NT = 256;
constexpr int BAND = 16;                  // macroblock rows of a band of the analyse kernel: one wave each
constexpr int META = MAF_VP8_ENC_META_WORDS;
constexpr int ZZ[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};       // k_vp8_zigzag, for unrolled loops
__constant__ uint8_t k_inv_zigzag[16] = {0, 1, 5, 6, 2, 4, 7, 12, 3, 8, 11, 13, 9, 10, 14, 15};

typedef maf_vp8_enc_job_t Job;

struct Planes {
    uint8_t *y, *u, *v;
    int64_t ys, cs;                       // row pitch of luma / chroma
};
__host__ __device__ inline int64_t plane_bytes_of(int mbw, int mbh) { return 384 * (int64_t)mbw * mbh; }
__device__ inline Planes planes_of(uint8_t* base, const Job& j) {
    Planes p;
    const int64_t n = (int64_t)j.mbw * j.mbh;
    p.y = base + j.plane_off;
    p.u = p.y + 256 * n;
    p.v = p.u + 64 * n;
    p.ys = 16 * (int64_t)j.mbw;
    p.cs = 8 * (int64_t)j.mbw;
    return p;
}

// macroblock rows of token partition p of n: rows p, p + n, ...
__host__ __device__ inline int part_rows(int mbh, int n, int p) { return (mbh - p + n - 1) / n; }
// the partitions' places inside a file's region of parts: idx 0 = the first partition, 1 + p = token partition p
__host__ __device__ inline int64_t part_cap(const Job& j, int idx) {
    const int n = 1 << j.log2_parts;
    return idx == 0 ? MAF_VP8_ENC_P0_BOUND((int64_t)j.mbw * j.mbh) : MAF_VP8_ENC_PART_BOUND((int64_t)j.mbw * part_rows(j.mbh, n, idx - 1));
}
__host__ __device__ inline int64_t part_begin(const Job& j, int idx) {
    int64_t at = 0;
    for (int i = 0; i < idx; ++i) at += part_cap(j, i);
    return at;
}
// what a file can take: its frame, the first partition, the size table, the partitions, the pad byte
__host__ __device__ inline int64_t file_bound(const Job& j) {
    const int n = 1 << j.log2_parts;
    return MAF_VP8_ENC_FILE_BYTES + MAF_VP8_ENC_FRAME_BYTES + part_begin(j, n + 1) + 3 * (n - 1) + 1;
}

// the lanes of ONE wave: LDS written by some of them is read by others behind this
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
__device__ inline int wave_sum(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// ---------------------------------------------------------------- CONVERT

__global__ __launch_bounds__(NT) void vp8_enc_convert_kernel(const Job* jobs, uint8_t* planes) {
    const Job j = jobs[blockIdx.y];
    const int cw = 8 * j.mbw;
    const int64_t c = (int64_t)blockIdx.x * NT + threadIdx.x;
    if (c >= 64 * (int64_t)j.mbw * j.mbh) return;
    const int cy = (int)(c / cw), cx = (int)(c % cw);
    const Planes pl = planes_of(planes, j);
    const uint8_t* src = static_cast<const uint8_t*>(j.src);
    int r4 = 0, g4 = 0, b4 = 0;
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const int y = min(2 * cy + dy, j.h - 1);             // the last row and column replicate
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const int x = min(2 * cx + dx, j.w - 1);
            const uint8_t* p = src + y * j.pitch + 3 * (int64_t)x;
            const int b = p[0], g = p[1], r = p[2];
            pl.y[(2 * cy + dy) * pl.ys + 2 * cx + dx] = (uint8_t)vp8e_luma(r, g, b);
            r4 += r; g4 += g; b4 += b;
        }
    }
    pl.u[cy * pl.cs + cx] = (uint8_t)vp8e_chroma_u(r4, g4, b4);
    pl.v[cy * pl.cs + cx] = (uint8_t)vp8e_chroma_v(r4, g4, b4);
}

// ---------------------------------------------------------------- ANALYSE

struct Quant {
    int y1dc, y1ac, y2dc, y2ac, uvdc, uvac;
};
__device__ inline Quant quant_of(int q) {
    Quant k;
    k.y1dc = k_vp8_dc_q[q];
    k.y1ac = k_vp8_ac_q[q];
    k.y2dc = k_vp8_dc_q[q] * 2;
    k.y2ac = max((k_vp8_ac_q[q] * 101581) >> 16, 8);
    k.uvdc = k_vp8_dc_q[min(q, 117)];
    k.uvac = k_vp8_ac_q[q];
    return k;
}

struct alignas(16) Tile {                  // one wave's work space
    uint8_t src[384];                     // Y 16 x 16, U 8 x 8, V 8 x 8
    uint8_t ey[36], eu[20], ev[20];       // the corner, the samples above, the samples to the left
    int16_t dc[16];                       // the luma blocks' DC, then their dequantised DC
    int16_t y2[16];                       // the dequantised Y2 coefficients in raster order
};

// One macroblock by one wave -> true where it has no level at all
__device__ inline bool analyse_mb(Tile& t, const Planes& in, const Planes& rc, const Quant& q, int mx, int my, int lane, int16_t* levels, uint32_t* info) {
    // the source samples and the reconstructed neighbours
    {
        const int row = lane >> 2, col = (lane & 3) * 4;
        *reinterpret_cast<uint32_t*>(t.src + 16 * row + col) = *reinterpret_cast<const uint32_t*>(in.y + (16 * (int64_t)my + row) * in.ys + 16 * mx + col);
        if (lane < 32) {
            const int k = lane & 15, crow = k >> 1, ccol = (k & 1) * 4;
            const uint8_t* p = (lane < 16 ? in.u : in.v) + (8 * (int64_t)my + crow) * in.cs + 8 * mx + ccol;
            *reinterpret_cast<uint32_t*>(t.src + 256 + 64 * (lane >> 4) + 8 * crow + ccol) = *reinterpret_cast<const uint32_t*>(p);
        }
        for (int i = lane; i < 33 + 17 + 17; i += 64) {
            const int pi = i < 33 ? 0 : i < 50 ? 1 : 2, k = i - (pi == 0 ? 0 : pi == 1 ? 33 : 50), n = pi == 0 ? 16 : 8;
            const uint8_t* P = pi == 0 ? rc.y : pi == 1 ? rc.u : rc.v;
            const int64_t ps = pi == 0 ? rc.ys : rc.cs, x0 = (int64_t)n * mx, y0 = (int64_t)n * my;
            int v;
            if (k == 0) v = my ? (mx ? P[(y0 - 1) * ps + x0 - 1] : 129) : 127;
            else if (k <= n) v = my ? P[(y0 - 1) * ps + x0 + k - 1] : 127;
            else v = mx ? P[(y0 + k - n - 1) * ps + x0 - 1] : 129;
            (pi == 0 ? t.ey : pi == 1 ? t.eu : t.ev)[k] = (uint8_t)v;
        }
    }
    wave_sync();
    const int dcy = vp8e_dc(t.ey, 16, mx > 0, my > 0), dcu = vp8e_dc(t.eu, 8, mx > 0, my > 0), dcv = vp8e_dc(t.ev, 8, mx > 0, my > 0);
    // the squared error of the four candidates: luma, four samples a lane; chroma, two samples a lane over U and V together
    int ymode = 0, uvmode = 0;
    {
        int sy[4] = {0, 0, 0, 0}, sc[4] = {0, 0, 0, 0};
        const int row = lane >> 2, col = (lane & 3) * 4;
        const int pc = lane >> 5, ci = (lane & 31) * 2, crow = ci >> 3, ccol = ci & 7;
        const uint8_t* ec = pc ? t.ev : t.eu;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int d = t.src[16 * row + col + k] - vp8e_pred(m, t.ey, 16, col + k, row, dcy);
                sy[m] += d * d;
            }
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int d = t.src[256 + 64 * pc + 8 * crow + ccol + k] - vp8e_pred(m, ec, 8, ccol + k, crow, pc ? dcv : dcu);
                sc[m] += d * d;
            }
        }
        int besty = 0, bestc = 0;
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int a = wave_sum(sy[m]), b = wave_sum(sc[m]);
            if (m == 0 || a < besty) { besty = a; ymode = m; }                // ties: the lowest number
            if (m == 0 || b < bestc) { bestc = b; uvmode = m; }
        }
    }
    // a lane per 4x4 block: 0 .. 15 luma, 16 .. 19 U, 20 .. 23 V
    const bool luma = lane < 16, block = lane < 24;
    const int pi = luma ? 0 : lane < 20 ? 1 : 2;
    const int bb = luma ? lane : (lane - 16) & 3;
    const int r0 = luma ? 4 * (bb >> 2) : 4 * (bb >> 1), c0 = luma ? 4 * (bb & 3) : 4 * (bb & 1);
    const int n = luma ? 16 : 8, mode = luma ? ymode : uvmode, dcv_ = pi == 0 ? dcy : pi == 1 ? dcu : dcv;
    const uint8_t* e = pi == 0 ? t.ey : pi == 1 ? t.eu : t.ev;
    const uint8_t* s = t.src + (pi == 0 ? 0 : pi == 1 ? 256 : 320);
    int pred[16], co[16];
    if (block) {
        int res[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            pred[k] = vp8e_pred(mode, e, n, c0 + (k & 3), r0 + (k >> 2), dcv_);
            res[k] = s[n * (r0 + (k >> 2)) + c0 + (k & 3)] - pred[k];
        }
        vp8e_fdct(res, co);
        if (luma) t.dc[lane] = (int16_t)co[0];
    }
    wave_sync();
    // the Y2 block: lane o gives coefficient o (raster order) of the forward WHT, its level and what a decoder makes of it
    int y2_level = 0;
    if (luma) {
        const int c = vp8e_fwht(t.dc, lane);
        y2_level = vp8e_quantise(c, lane ? q.y2ac : q.y2dc);
        t.y2[lane] = (int16_t)(y2_level * (lane ? q.y2ac : q.y2dc));
        levels[24 * 16 + k_inv_zigzag[lane]] = (int16_t)y2_level;
    }
    const uint64_t y2_any = __ballot(luma && y2_level != 0);
    wave_sync();
    bool any = false;
    if (block) {
        const int qdc = luma ? q.y1dc : q.uvdc, qac = luma ? q.y1ac : q.uvac;
        int16_t deq[16];
        int16_t* lv = levels + 16 * lane;
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int level = (k == 0 && luma) ? 0 : vp8e_quantise(co[ZZ[k]], k ? qac : qdc);
            lv[k] = (int16_t)level;
            deq[ZZ[k]] = (int16_t)(level * (k ? qac : qdc));
            any |= level != 0;
        }
        if (luma) deq[0] = (int16_t)vp8_iwht(t.y2, lane);
        uint8_t* P = (pi == 0 ? rc.y : pi == 1 ? rc.u : rc.v) + ((int64_t)n * my + r0) * (pi == 0 ? rc.ys : rc.cs) + n * mx + c0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int r[4];
            vp8_idct_row(deq, i, r);
            const uint32_t px = (uint32_t)vp8_clip255(pred[4 * i] + r[0]) | (uint32_t)vp8_clip255(pred[4 * i + 1] + r[1]) << 8 |
                                (uint32_t)vp8_clip255(pred[4 * i + 2] + r[2]) << 16 | (uint32_t)vp8_clip255(pred[4 * i + 3] + r[3]) << 24;
            *reinterpret_cast<uint32_t*>(P + i * (pi == 0 ? rc.ys : rc.cs)) = px;
        }
    }
    const uint64_t nz = __ballot(block && any);
    const uint32_t bits = (uint32_t)(nz & 0xffffff) | (y2_any ? 1u << 24 : 0u);
    if (lane == 0) *info = bits | (uint32_t)ymode << 25 | (uint32_t)uvmode << 27 | (bits ? 0u : 1u << 29);
    return bits == 0;
}

__global__ __launch_bounds__(64 * BAND) void vp8_enc_analyse_kernel(const Job* jobs, int base_q, uint8_t* planes, uint8_t* recon, int16_t* levels, uint32_t* info,
                                                                     int32_t* meta) {
    __shared__ Tile tiles[BAND];
    __shared__ int skipped;
    const Job j = jobs[blockIdx.x];
    const Planes in = planes_of(planes, j), rc = planes_of(recon, j);
    const Quant q = quant_of(base_q);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mbw = j.mbw, mbh = j.mbh;
    if (threadIdx.x == 0) skipped = 0;
    int zero = 0;
    for (int y0 = 0; y0 < mbh; y0 += BAND) {
        const int rows = min(BAND, mbh - y0), steps = mbw + rows - 1;
        const int my = y0 + wave;
        for (int t = 0; t < steps; ++t) {                      // the same count for every wave: the barrier below is reached by all
            const int mx = t - wave;                           // (mx, my) needs (mx - 1, my), (mx, my - 1), (mx - 1, my - 1): one macroblock behind
            if (wave < rows && mx >= 0 && mx < mbw) {
                const int64_t mb = j.mb0 + (int64_t)my * mbw + mx;
                zero += analyse_mb(tiles[wave], in, rc, q, mx, my, lane, levels + mb * MAF_VP8_ENC_MB_LEVELS, info + mb);
            }
            __threadfence_block();
            __syncthreads();
        }
    }
    if (lane == 0 && zero) atomicAdd(&skipped, zero);
    __syncthreads();
    if (threadIdx.x == 0) meta[META * blockIdx.x] = skipped;
}

// ---------------------------------------------------------------- TOKENS

// RFC 6386 section 7.3, as webp_lossy_ref.BoolEncoder: a carry walks back through the partition's own bytes
struct BoolWriter {
    uint8_t* out;
    int64_t cap, pos;
    uint32_t range, bottom;
    int count, overflow;
};
__device__ inline void bw_init(BoolWriter& w, uint8_t* out, int64_t cap) {
    w.out = out; w.cap = cap; w.pos = 0; w.range = 255; w.bottom = 0; w.count = 24; w.overflow = 0;
}
__device__ inline void bw_byte(BoolWriter& w, uint32_t v) {
    if (w.pos < w.cap) w.out[w.pos] = (uint8_t)v; else w.overflow = 1;
    ++w.pos;
}
__device__ inline void bw_carry(BoolWriter& w) {
    int64_t i = min(w.pos, w.cap) - 1;
    while (i >= 0 && w.out[i] == 255) w.out[i--] = 0;
    if (i >= 0) ++w.out[i];
}
__device__ inline void bw_put(BoolWriter& w, int prob, bool b) {
    const uint32_t split = 1 + (((w.range - 1) * (uint32_t)prob) >> 8);
    if (b) { w.bottom += split; w.range -= split; } else w.range = split;
    while (w.range < 128) {                                    // at most 7 times
        w.range <<= 1;
        if (w.bottom & 0x80000000u) bw_carry(w);
        w.bottom <<= 1;
        if (--w.count == 0) {
            bw_byte(w, w.bottom >> 24);
            w.bottom &= 0xffffffu;
            w.count = 8;
        }
    }
}
__device__ inline void bw_value(BoolWriter& w, int n, int x) {
    for (int i = n - 1; i >= 0; --i) bw_put(w, 128, (x >> i) & 1);
}
__device__ inline int64_t bw_finish(BoolWriter& w) {
    const int c = w.count;
    uint32_t v = w.bottom;
    if (v & (1u << (32 - c))) bw_carry(w);
    v <<= c & 7;
    for (int i = 0; i < (c >> 3); ++i) v <<= 8;
    for (int i = 0; i < 4; ++i) { bw_byte(w, v >> 24); v <<= 8; }
    return w.pos;
}

// 16 levels in registers, two to a word (one 32-byte read per block instead of a read per bool): level n by selects, no indexing
struct Levels {
    uint4 lo, hi;
    __device__ inline int operator[](int n) const {
        const int k = n >> 1;
        const uint32_t v = k == 0 ? lo.x : k == 1 ? lo.y : k == 2 ? lo.z : k == 3 ? lo.w : k == 4 ? hi.x : k == 5 ? hi.y : k == 6 ? hi.z : hi.w;
        return (int16_t)(v >> (16 * (n & 1)));
    }
};

// the tokens of one block: webp_lossy_ref.walk_coeffs as a writer.  levels: 16 levels in zigzag order, 16-byte aligned
__device__ inline void put_block(BoolWriter& w, int type, int ctx, int first, const int16_t* levels) {
    const Levels lv = {*reinterpret_cast<const uint4*>(levels), *reinterpret_cast<const uint4*>(levels + 8)};
    int last = first;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if (i >= first && lv[i]) last = i + 1;
    int n = first;
    const uint8_t* P = k_vp8_coeff_proba0 + 264 * type;
    const uint8_t* p = P + 33 * k_vp8_bands[n] + 11 * ctx;
    while (n < 16) {
        bw_put(w, p[0], n < last);
        if (n >= last) return;
        while (lv[n] == 0) {                                   // ends: lv[last - 1] is not zero
            bw_put(w, p[1], false);
            ++n;
            p = P + 33 * k_vp8_bands[n];
        }
        bw_put(w, p[1], true);
        const int v = lv[n], a = v < 0 ? -v : v;
        int nxt = 1;
        bw_put(w, p[2], a > 1);
        if (a > 1) {
            nxt = 2;
            bw_put(w, p[3], a > 4);
            if (a <= 4) {
                bw_put(w, p[4], a > 2);
                if (a > 2) bw_put(w, p[5], a == 4);
            } else {
                bw_put(w, p[6], a > 10);
                if (a <= 10) {
                    bw_put(w, p[7], a > 6);
                    if (a <= 6) {
                        bw_put(w, 159, a == 6);
                    } else {
                        bw_put(w, 165, a >= 9);
                        bw_put(w, 145, (a - 7) & 1);
                    }
                } else {
                    const int cat = a < 19 ? 0 : a < 35 ? 1 : a < 67 ? 2 : 3;
                    bw_put(w, p[8], cat >= 2);
                    bw_put(w, p[9 + (cat >> 1)], cat & 1);
                    const int bits = cat == 3 ? 11 : 3 + cat, extra = a - 3 - (8 << cat);
                    for (int i = 0; i < bits; ++i) bw_put(w, k_vp8_cat3456[cat][i], (extra >> (bits - 1 - i)) & 1);
                }
            }
        }
        bw_put(w, 128, v < 0);
        ++n;
        p = P + 33 * k_vp8_bands[n] + 11 * nxt;
    }
}

__device__ inline int skip_proba_of(int total, int skips) { return (int)(((int64_t)(total - skips) * 255) / total); }

// blockIdx.y = 0: the first partition (header, modes); 1 + p: token partition p.  One chain of bools: lane 0 runs it.
__global__ __launch_bounds__(64) void vp8_enc_tokens_kernel(const Job* jobs, int base_q, int level, const int16_t* levels, const uint32_t* info, int32_t* meta,
                                                            uint8_t* parts) {
    const Job j = jobs[blockIdx.x];
    const int idx = blockIdx.y, n_parts = 1 << j.log2_parts;
    if (idx > n_parts || threadIdx.x != 0) return;
    const int mbw = j.mbw, mbh = j.mbh, total = mbw * mbh;
    int32_t* m = meta + META * blockIdx.x;
    const int skip_proba = skip_proba_of(total, m[0]);
    const bool use_skip = skip_proba < 250;
    const uint32_t* inf = info + j.mb0;
    BoolWriter w;
    bw_init(w, parts + j.part_off + part_begin(j, idx), part_cap(j, idx));
    if (idx == 0) {
        bw_value(w, 4, 0);                                     // colorspace, clamp, no segments, the normal filter
        bw_value(w, 6, level);
        bw_value(w, 3, 0);                                     // sharpness
        bw_put(w, 128, false);                                 // no filter deltas
        bw_value(w, 2, j.log2_parts);
        bw_value(w, 7, base_q);
        bw_value(w, 5, 0);                                     // no dq
        bw_put(w, 128, false);                                 // refresh
        for (int i = 0; i < 1056; ++i) bw_put(w, k_vp8_coeff_update[i], false);
        bw_put(w, 128, use_skip);
        if (use_skip) bw_value(w, 8, skip_proba);
        for (int i = 0; i < total; ++i) {
            const uint32_t f = inf[i];
            const int ym = (f >> 25) & 3, um = (f >> 27) & 3;
            if (use_skip) bw_put(w, skip_proba, (f >> 29) & 1);
            bw_put(w, 145, true);                              // predicted 16x16
            const bool tm_h = ym == 1 || ym == 3;
            bw_put(w, 156, tm_h);
            if (tm_h) bw_put(w, 128, ym == 1); else bw_put(w, 163, ym == 2);
            bw_put(w, 142, um != 0);
            if (um != 0) {
                bw_put(w, 114, um != 2);
                if (um != 2) bw_put(w, 183, um == 1);
            }
        }
    } else {
        for (int my = idx - 1; my < mbh; my += n_parts) {
            uint32_t left = 0;
            for (int mx = 0; mx < mbw; ++mx) {
                const int64_t mb = (int64_t)my * mbw + mx;
                const uint32_t f = inf[mb] & 0x1ffffff, top = my ? inf[mb - mbw] & 0x1ffffff : 0;
                if (!(use_skip && f == 0)) {
                    const int16_t* lv = levels + (j.mb0 + mb) * MAF_VP8_ENC_MB_LEVELS;
                    put_block(w, 1, (int)((top >> 24) & 1) + (int)((left >> 24) & 1), 0, lv + 24 * 16);
                    for (int y = 0; y < 4; ++y)
                        for (int x = 0; x < 4; ++x) {
                            const int t = y ? (f >> (4 * (y - 1) + x)) & 1 : (top >> (12 + x)) & 1;
                            const int l = x ? (f >> (4 * y + x - 1)) & 1 : (left >> (4 * y + 3)) & 1;
                            put_block(w, 0, t + l, 1, lv + 16 * (4 * y + x));
                        }
                    for (int ch = 0; ch < 2; ++ch)
                        for (int y = 0; y < 2; ++y)
                            for (int x = 0; x < 2; ++x) {
                                const int b0 = 16 + 4 * ch;
                                const int t = y ? (f >> (b0 + x)) & 1 : (top >> (b0 + 2 + x)) & 1;
                                const int l = x ? (f >> (b0 + 2 * y)) & 1 : (left >> (b0 + 2 * y + 1)) & 1;
                                put_block(w, 2, t + l, 0, lv + 16 * (b0 + 2 * y + x));
                            }
                }
                left = f;
            }
        }
    }
    m[2 + idx] = (int32_t)bw_finish(w);
    if (w.overflow) atomicOr(&m[1], MAF_VP8_ENC_ST_OVERFLOW);
}

// ---------------------------------------------------------------- OFFSETS, ASSEMBLE

__device__ inline int64_t payload_of(const Job& j, const int32_t* m) {
    const int n = 1 << j.log2_parts;
    int64_t bytes = MAF_VP8_ENC_FRAME_BYTES + 3 * (n - 1);
    for (int i = 0; i <= n; ++i) bytes += m[2 + i];
    return bytes;
}

__global__ __launch_bounds__(NT) void vp8_enc_offsets_kernel(const Job* jobs, int n_files, const int32_t* meta, int32_t* lengths, int64_t* offsets) {
    __shared__ int64_t sh[NT];
    int64_t carry = 0;
    for (int f0 = 0; f0 < n_files; f0 += NT) {
        const int f = f0 + threadIdx.x;
        int64_t len = 0;
        if (f < n_files) {
            const int32_t* m = meta + META * f;
            const int64_t payload = payload_of(jobs[f], m);
            len = m[1] || m[2] >= MAF_VP8_ENC_MAX_P0 ? 0 : MAF_VP8_ENC_FILE_BYTES + payload + (payload & 1);
            lengths[f] = (int32_t)len;
        }
        const int64_t before = block_excl_sum<NT>(len, sh);
        if (f < n_files) offsets[f] = carry + before;
        if (threadIdx.x == NT - 1) sh[0] = before + len;
        __syncthreads();
        carry += sh[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void vp8_enc_assemble_kernel(const Job* jobs, const int32_t* meta, const uint8_t* parts, const int32_t* lengths,
                                                              const int64_t* offsets, uint8_t* out, int64_t out_bytes) {
    const Job j = jobs[blockIdx.x];
    const int32_t* m = meta + META * blockIdx.x;
    if (lengths[blockIdx.x] == 0) return;                      // the whole workgroup
    const int n = 1 << j.log2_parts;
    const int64_t o = offsets[blockIdx.x], payload = payload_of(j, m);
    auto put = [&](int64_t at, uint32_t v) {
        if (at >= 0 && at < out_bytes) out[at] = (uint8_t)v;
    };
    if (threadIdx.x == 0) {
        const uint32_t riff = (uint32_t)(12 + payload + (payload & 1)), size = (uint32_t)payload, tag = 1u << 4 | (uint32_t)m[2] << 5;
        const uint8_t head[30] = {'R', 'I', 'F', 'F', (uint8_t)riff, (uint8_t)(riff >> 8), (uint8_t)(riff >> 16), (uint8_t)(riff >> 24), 'W', 'E', 'B', 'P',
                                  'V', 'P', '8', ' ', (uint8_t)size, (uint8_t)(size >> 8), (uint8_t)(size >> 16), (uint8_t)(size >> 24),
                                  (uint8_t)tag, (uint8_t)(tag >> 8), (uint8_t)(tag >> 16), 0x9d, 0x01, 0x2a,
                                  (uint8_t)j.w, (uint8_t)(j.w >> 8), (uint8_t)j.h, (uint8_t)(j.h >> 8)};
        for (int i = 0; i < 30; ++i) put(o + i, head[i]);
        const int64_t table = o + 30 + m[2];
        for (int p = 0; p + 1 < n; ++p) {
            const uint32_t s = (uint32_t)m[3 + p];
            put(table + 3 * p, s); put(table + 3 * p + 1, s >> 8); put(table + 3 * p + 2, s >> 16);
        }
        if (payload & 1) put(o + MAF_VP8_ENC_FILE_BYTES + payload, 0);
    }
    int64_t at = o + 30;
    for (int idx = 0; idx <= n; ++idx) {
        const uint8_t* src = parts + j.part_off + part_begin(j, idx);
        const int64_t len = min((int64_t)m[2 + idx], part_cap(j, idx));
        for (int64_t i = threadIdx.x; i < len; i += NT) put(at + i, src[i]);
        at += len + (idx == 0 ? 3 * (n - 1) : 0);
    }
}

}  // namespace

extern "C" int maf_vp8_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "vp8_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_vp8_enc_header_t); out[1] = (int32_t)sizeof(maf_vp8_enc_job_t);
    return 0;
}

extern "C" int maf_vp8_encode(const void* blob_host, const void* blob_dev, uint8_t* planes, uint8_t* recon, int16_t* levels, uint32_t* info, int32_t* meta,
                              uint8_t* parts, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_vp8_enc_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && planes && recon && levels && info && meta && parts && out && lengths && offsets, "vp8_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, planes, recon, levels}) && maf_aligned({offsets}, 8) && maf_aligned({info, meta, lengths}, 4),
                "vp8_encode: blob, planes, recon and levels must be 16-byte aligned, offsets 8-byte aligned, the 32-bit buffers 4-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_vp8_enc_header_t hd = maf_blob_header<maf_vp8_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files), "vp8_encode: 1 to 65535 files per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "vp8_encode: blob size out of range");
    MAF_REQUIRE(hd.base_q >= 0 && hd.base_q <= 127 && hd.level >= 0 && hd.level <= 63, "vp8_encode: base_q is 0 to 127, the filter level 0 to 63");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(Job), T), "vp8_encode: the job table lies outside the blob");
    const Job* jobs = reinterpret_cast<const Job*>(hb + hd.jobs_off);
    int64_t at_plane = 0, at_part = 0, at_mb = 0, need = 0, max_chroma = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const Job& j = jobs[i];
        MAF_REQUIRE(j.src, "vp8_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= MAF_VP8_ENC_MAX_SIDE && j.h <= MAF_VP8_ENC_MAX_SIDE, "vp8_encode: width and height are 1 to 16383");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "vp8_encode: a row pitch below 3 * width");
        MAF_REQUIRE(j.mbw == (j.w + 15) >> 4 && j.mbh == (j.h + 15) >> 4, "vp8_encode: mbw and mbh are ceil(w / 16) and ceil(h / 16)");
        const int64_t n = (int64_t)j.mbw * j.mbh;
        MAF_REQUIRE(MAF_VP8_ENC_P0_BOUND(n) < MAF_VP8_ENC_MAX_P0, "vp8_encode: too many macroblocks for the 19 bits of the first partition's size");
        MAF_REQUIRE(j.log2_parts >= 0 && j.log2_parts <= 3 && (1 << j.log2_parts) <= j.mbh, "vp8_encode: log2_parts is 0 to 3 and every partition owns a macroblock row");
        MAF_REQUIRE(j.plane_off == at_plane && j.mb0 == at_mb, "vp8_encode: the files' planes and macroblocks must follow each other");
        MAF_REQUIRE(j.part_off == at_part && j.part_bytes >= part_begin(j, (1 << j.log2_parts) + 1),
                    "vp8_encode: the partition regions must follow each other, none smaller than the bound");
        at_plane += (plane_bytes_of(j.mbw, j.mbh) + 15) / 16 * 16;
        at_part += j.part_bytes;
        at_mb += n;
        need += file_bound(j);
        max_chroma = 64 * n > max_chroma ? 64 * n : max_chroma;
    }
    MAF_REQUIRE(hd.plane_bytes >= at_plane && hd.n_mbs == at_mb && hd.part_bytes >= at_part && hd.out_bytes >= need && hd.max_chroma == max_chroma,
                "vp8_encode: a device buffer is smaller than the worst case, or a header count differs from the jobs' sum");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const Job* d_jobs = reinterpret_cast<const Job*>(db + hd.jobs_off);
    const int rc = maf_check_hip(hipMemsetAsync(meta, 0, (size_t)hd.n_files * META * sizeof(int32_t), s), "vp8_encode memset meta");
    if (rc) return rc;
    hipLaunchKernelGGL(vp8_enc_convert_kernel, dim3((unsigned)((max_chroma + NT - 1) / NT), hd.n_files), dim3(NT), 0, s, d_jobs, planes);
    MAF_LAUNCH_CHECK("vp8_enc_convert");
    hipLaunchKernelGGL(vp8_enc_analyse_kernel, dim3(hd.n_files), dim3(64 * BAND), 0, s, d_jobs, hd.base_q, planes, recon, levels, info, meta);
    MAF_LAUNCH_CHECK("vp8_enc_analyse");
    hipLaunchKernelGGL(vp8_enc_tokens_kernel, dim3(hd.n_files, 9), dim3(64), 0, s, d_jobs, hd.base_q, hd.level, levels, info, meta, parts);
    MAF_LAUNCH_CHECK("vp8_enc_tokens");
    hipLaunchKernelGGL(vp8_enc_offsets_kernel, dim3(1), dim3(NT), 0, s, d_jobs, hd.n_files, meta, lengths, offsets);
    MAF_LAUNCH_CHECK("vp8_enc_offsets");
    hipLaunchKernelGGL(vp8_enc_assemble_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, meta, parts, lengths, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("vp8_enc_assemble");
    return 0;
}
