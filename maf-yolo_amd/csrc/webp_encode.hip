// Lossless WebP (VP8L) encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any row pitch), RIFF / WEBP
// files out that libwebp and csrc/webp_decode.hip decode to the pixels that went in.  Replaces the final cv2.imwrite of Inferer.infer
// (yolov6/core/inferer.py) for a .webp source.  The stream (subtract-green, the predictor transform with a mode per block, copies at distance
// 1 from a closed-form run rule, five length-limited Huffman codes per image) is restated rule by rule in tests/webp_encode_ref.py; the trees
// are csrc/png_trees.h; the host side (sizes, the job and image tables) is maf-yolo_amd/webp_encode.py; include/mafyolo_webp_encode.h lists the
// kernels, the blob and the buffers.
//
// Every index that depends on pixel content (token counts, bit offsets, lengths) is bounded by construction (a token covers at least one
// pixel; MAF_WEBP_ENC_BOUND) and compared with its region's size before a store all the same.
#include "maf_common.h"
#include "../../include/mafyolo_webp_encode.h"
#include "image_blob.h"
#include "block_scan.h"
#include "png_trees.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MAF_WEBP_ENC_CHUNK;
constexpr int ITEMS = CHUNK / NT;
constexpr int NONE_AFTER = 0x7FFFFFFF;
constexpr int CW = MAF_WEBP_ENC_CODE_WORDS, HW = MAF_WEBP_ENC_HEAD_WORDS, NCODES = MAF_WEBP_ENC_CODES;
constexpr int MAXCOPY = MAF_WEBP_ENC_MAX_COPY;
constexpr uint32_t COPY = 0x80000000u;
static_assert(ITEMS == 4, "a thread owns 4 pixels (one 16-byte vector) or 4 tokens of a chunk");
static_assert(CW <= png_trees::L_CODES && HW * 32 >= 1 + 4 + 19 * 3 + 1 + 7 * CW, "png_trees::Work holds the alphabet; a description fits its words");

typedef maf_webp_enc_job_t Job;
typedef maf_webp_enc_image_t Image;

// the last entry whose first chunk (block, ...) is at most i
template <typename F>
__device__ __forceinline__ int entry_of(int n, int i, F first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive scan under `op` (identity `ident`) in the order of `at` (a permutation of 0 .. NT - 1: at = tid scans forward, NT - 1 - tid backward)
template <typename T, typename Op>
__device__ T block_excl_scan(T v, T ident, int at, T* sh, Op op) {
    sh[at] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const T t = at >= d ? op(sh[at - d], sh[at]) : sh[at];
        __syncthreads();
        sh[at] = t;
        __syncthreads();
    }
    const T r = at ? sh[at - 1] : ident;
    __syncthreads();
    return r;
}

// exclusive scan of in[0 .. n) into out64 or out32 by ONE workgroup (in == out32 is fine); returns the total
__device__ __forceinline__ int64_t scan_by_one_workgroup(const int32_t* in, int64_t* out64, int32_t* out32, int n, int64_t* sh) {
    int64_t carry = 0;
    for (int t0 = 0; t0 < n; t0 += NT) {
        const int i = t0 + threadIdx.x;
        const int64_t v = i < n ? (int64_t)in[i] : 0;
        const int64_t before = block_excl_sum<NT>(v, sh);
        if (i < n) {
            if (out64) out64[i] = carry + before; else out32[i] = (int32_t)(carry + before);
        }
        if (threadIdx.x == NT - 1) sh[0] = before + v;
        __syncthreads();
        carry += sh[0];
        __syncthreads();
    }
    return carry;
}

// ---- the transforms.  avg2, clip255 and predict are csrc/webp_decode.hip's, restated: the decoder adds what this file subtracts.
__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
__device__ __forceinline__ uint32_t sub_px(uint32_t a, uint32_t b) {
    return (((a | 0x00FF00FFu) - (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a | 0xFF00FF00u) - (b & 0x00FF00FFu)) & 0x00FF00FFu);
}
__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__device__ __forceinline__ uint32_t predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return avg2(avg2(L, TR), T);
        case 6: return avg2(L, TL);
        case 7: return avg2(L, T);
        case 8: return avg2(TL, T);
        case 9: return avg2(T, TR);
        case 10: return avg2(avg2(L, TL), avg2(T, TR));
        case 11: {
            int dt = 0, dl = 0;
#pragma unroll
            for (int s = 0; s < 32; s += 8) {
                const int c = (int)(TL >> s) & 255;
                dt += abs(((int)(T >> s) & 255) - c);
                dl += abs(((int)(L >> s) & 255) - c);
            }
            return dt < dl ? L : T;
        }
        case 12: {
            uint32_t o = 0;
#pragma unroll
            for (int s = 0; s < 32; s += 8) o |= (uint32_t)clip255(((int)(L >> s) & 255) + ((int)(T >> s) & 255) - ((int)(TL >> s) & 255)) << s;
            return o;
        }
        case 13: {
            const uint32_t A = avg2(L, T);
            uint32_t o = 0;
#pragma unroll
            for (int s = 0; s < 32; s += 8) {
                const int a = (int)(A >> s) & 255, c = (int)(TL >> s) & 255;
                o |= (uint32_t)clip255(a + (a - c) / 2) << s;             // C division: toward zero
            }
            return o;
        }
        default: return 0xFF000000u;
    }
}

// min(v, 256 - v) summed over the R, G, B bytes of a residual
__device__ __forceinline__ int residual_cost(uint32_t r) {
    int c = 0;
#pragma unroll
    for (int s = 0; s < 24; s += 8) {
        const int v = (int)(r >> s) & 255;
        c += min(v, 256 - v);
    }
    return c;
}

__global__ __launch_bounds__(NT) void webp_enc_gather_kernel(const Job* jobs, const Image* images, int n_images, uint32_t* argb) {
    const int ch = blockIdx.x;
    const Image im = images[entry_of(n_images, ch, [&](int i) { return images[i].chunk0; })];
    if (!im.main) return;
    const Job j = jobs[im.file];
    const int64_t p0 = (int64_t)(ch - im.chunk0) * CHUNK + ITEMS * threadIdx.x;
    if (p0 >= im.n_px) return;
    uint32_t o[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int p = (int)p0 + i;
        o[i] = 0u;
        if (p < im.n_px) {
            const int y = p / j.w, x = p - y * j.w;
            const uint8_t* at = static_cast<const uint8_t*>(j.src) + (int64_t)y * j.pitch + 3 * x;
            const uint32_t b = at[0], g = at[1], r = at[2];
            o[i] = 0xFF000000u | (((r - g) & 255u) << 16) | (g << 8) | ((b - g) & 255u);
        }
    }
    const u32x4_t v = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<u32x4_t*>(argb + im.px_off + p0) = v;                       // the image's region is a multiple of 4 words
}

// one workgroup per block: every thread sums the 14 costs of its pixels, a wave reduces them across its lanes, LDS holds the four waves' sums
__global__ __launch_bounds__(NT) void webp_enc_modes_kernel(const Job* jobs, const Image* images, int n_files, const uint32_t* argb, int32_t* modes, uint32_t* px) {
    __shared__ int sh[NT / 64][14];
    const int b = blockIdx.x;
    const int f = entry_of(n_files, b, [&](int i) { return jobs[i].block0; });
    const Job j = jobs[f];
    const Image sub = images[2 * f], mainim = images[2 * f + 1];
    const int k = b - j.block0, by = k / j.bw, bx = k - by * j.bw;
    const int x0 = bx << j.bits, y0 = by << j.bits, bwid = min(1 << j.bits, j.w - x0), bhei = min(1 << j.bits, j.h - y0);
    const uint32_t* a = argb + mainim.px_off;
    int cost[14];
#pragma unroll
    for (int m = 0; m < 14; ++m) cost[m] = 0;
    for (int i = threadIdx.x; i < bwid * bhei; i += NT) {
        const int yy = i / bwid, x = x0 + i - yy * bwid, y = y0 + yy;
        if (x < 1 || y < 1) continue;                                            // row 0 and column 0 do not depend on the mode
        const int64_t p = (int64_t)y * j.w + x;
        const uint32_t C = a[p], L = a[p - 1], T = a[p - j.w], TL = a[p - j.w - 1], TR = a[p - j.w + 1];      // TR of the last column: this row's first pixel
#pragma unroll
        for (int m = 0; m < 14; ++m) cost[m] += residual_cost(sub_px(C, predict(m, L, T, TL, TR)));
    }
#pragma unroll
    for (int m = 0; m < 14; ++m) {
        int c = cost[m];
        for (int d = 32; d; d >>= 1) c += __shfl_down(c, d, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][m] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int best = 0, best_cost = 0x7FFFFFFF;
        for (int m = 0; m < 14; ++m) {
            int c = 0;
            for (int w = 0; w < NT / 64; ++w) c += sh[w][m];
            if (c < best_cost) { best_cost = c; best = m; }                      // a tie stays with the lower mode
        }
        modes[b] = best;
        if (k < sub.n_px) px[sub.px_off + k] = 0xFF000000u | ((uint32_t)best << 8);
    }
}

__global__ __launch_bounds__(NT) void webp_enc_residual_kernel(const Job* jobs, const Image* images, int n_images, const uint32_t* argb, const int32_t* modes,
                                                                uint32_t* px) {
    const int ch = blockIdx.x;
    const Image im = images[entry_of(n_images, ch, [&](int i) { return images[i].chunk0; })];
    if (!im.main) return;
    const Job j = jobs[im.file];
    const int64_t p0 = (int64_t)(ch - im.chunk0) * CHUNK + ITEMS * threadIdx.x;
    if (p0 >= im.n_px) return;
    const uint32_t* a = argb + im.px_off;
    uint32_t o[ITEMS];
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int p = (int)p0 + i;
        o[i] = 0u;
        if (p < im.n_px) {
            const int y = p / j.w, x = p - y * j.w;
            uint32_t pred;
            if (y == 0) pred = x == 0 ? 0xFF000000u : a[p - 1];
            else if (x == 0) pred = a[p - j.w];
            else pred = predict(modes[j.block0 + (y >> j.bits) * j.bw + (x >> j.bits)], a[p - 1], a[p - j.w], a[p - j.w - 1], a[p - j.w + 1]);
            o[i] = sub_px(a[p], pred);
        }
    }
    const u32x4_t v = {o[0], o[1], o[2], o[3]};
    *reinterpret_cast<u32x4_t*>(px + im.px_off + p0) = v;
}

// ---- the run rule, image by image.  chunks: int32 [6][n_chunks]: last run start in the chunk (-1), first (NONE_AFTER), last before the chunk,
// first behind it, tokens (then: first token), token bits
struct Starts {
    uint32_t v[ITEMS];
    uint32_t bits;                                                              // bit i: pixel p0 + i starts a run
};

__device__ __forceinline__ Starts load_starts(const uint32_t* px, int p0, int n) {
    Starts s;
    s.bits = 0u;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) s.v[i] = 0u;
    if (p0 < n) {
        const u32x4_t v = *reinterpret_cast<const u32x4_t*>(px + p0);
        uint32_t prev = p0 > 0 ? px[p0 - 1] : 0u;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            s.v[i] = v[i];
            if (p0 + i < n && (p0 + i == 0 || v[i] != prev)) s.bits |= 1u << i;
            prev = v[i];
        }
    }
    return s;
}

__global__ __launch_bounds__(NT) void webp_enc_marks_kernel(const Image* images, int n_images, int n_chunks, const uint32_t* px, int32_t* chunks) {
    __shared__ int sh_last, sh_first;
    const int ch = blockIdx.x;
    const Image im = images[entry_of(n_images, ch, [&](int i) { return images[i].chunk0; })];
    if (threadIdx.x == 0) { sh_last = -1; sh_first = NONE_AFTER; }
    __syncthreads();
    const int64_t p64 = (int64_t)(ch - im.chunk0) * CHUNK + ITEMS * threadIdx.x;
    const int p0 = p64 < im.n_px ? (int)p64 : im.n_px;
    const Starts s = load_starts(px + im.px_off, p0, im.n_px);
    if (s.bits) {
        atomicMax(&sh_last, p0 + 31 - __clz(s.bits));
        atomicMin(&sh_first, p0 + __ffs(s.bits) - 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        chunks[ch] = sh_last;
        chunks[n_chunks + ch] = sh_first;
    }
}

__global__ __launch_bounds__(NT) void webp_enc_runs_kernel(const Image* images, int n_chunks, int32_t* chunks) {
    __shared__ int sh[NT];
    const Image im = images[blockIdx.x];
    const int32_t* last = chunks + im.chunk0;
    const int32_t* first = chunks + n_chunks + im.chunk0;
    int32_t* before = chunks + 2 * n_chunks + im.chunk0;
    int32_t* after = chunks + 3 * n_chunks + im.chunk0;
    int carry = -1;
    for (int t0 = 0; t0 < im.n_chunks; t0 += NT) {                               // forward: the last run start before each chunk
        const int i = t0 + threadIdx.x;
        const int v = i < im.n_chunks ? last[i] : -1;
        const int ex = max(carry, block_excl_scan(v, -1, (int)threadIdx.x, sh, [](int x, int y) { return max(x, y); }));
        if (i < im.n_chunks) before[i] = ex;
        if (threadIdx.x == NT - 1) sh[0] = max(ex, v);
        __syncthreads();
        carry = sh[0];
        __syncthreads();
    }
    carry = im.n_px;
    for (int t0 = 0; t0 < im.n_chunks; t0 += NT) {                               // backward: the first run start behind each chunk (n_px: none)
        const int i = im.n_chunks - 1 - (t0 + (int)threadIdx.x);
        const int v = i >= 0 ? first[i] : NONE_AFTER;
        const int ex = min(carry, block_excl_scan(v, NONE_AFTER, (int)threadIdx.x, sh, [](int x, int y) { return min(x, y); }));
        if (i >= 0) after[i] = ex;
        if (threadIdx.x == NT - 1) sh[0] = min(ex, v);
        __syncthreads();
        carry = sh[0];
        __syncthreads();
    }
}

// A pixel p of a run [ps, pe) starts a token when it is the run's first pixel (a literal), or with k = p - ps - 1, r = pe - ps - 1, q = r / 4096,
// rem = r % 4096: k < 4096 q and k % 4096 == 0 (a copy of 4096), k == 4096 q and rem >= 3 (a copy of rem), k >= 4096 q and rem < 3 (a literal).
template <bool WRITE>
__global__ __launch_bounds__(NT) void webp_enc_tokens_kernel(const Image* images, int n_images, int n_chunks, const uint32_t* px, int32_t* chunks, uint32_t* tok) {
    __shared__ int sh[NT];
    const int ch = blockIdx.x;
    const Image im = images[entry_of(n_images, ch, [&](int i) { return images[i].chunk0; })];
    const int64_t p64 = (int64_t)(ch - im.chunk0) * CHUNK + ITEMS * threadIdx.x;
    const int n = im.n_px;
    const bool live = p64 < n;
    const int p0 = live ? (int)p64 : n;
    const Starts s = load_starts(px + im.px_off, p0, n);
    const int mine_last = s.bits ? p0 + 31 - __clz(s.bits) : -1, mine_first = s.bits ? p0 + __ffs(s.bits) - 1 : NONE_AFTER;
    int ps = max(chunks[2 * n_chunks + ch], block_excl_scan(mine_last, -1, (int)threadIdx.x, sh, [](int x, int y) { return max(x, y); }));
    const int behind = min(chunks[3 * n_chunks + ch], block_excl_scan(mine_first, NONE_AFTER, NT - 1 - (int)threadIdx.x, sh, [](int x, int y) { return min(x, y); }));
    uint32_t symbols = 0u;                                                      // bit i: pixel p0 + i starts a token
    uint32_t lens[ITEMS];
    if (live) {
        int pe = min(behind, n);
        int ends[ITEMS];
#pragma unroll
        for (int i = ITEMS - 1; i >= 0; --i) {
            ends[i] = pe;
            if ((s.bits >> i) & 1u) pe = p0 + i;
        }
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) {
            const int p = p0 + i;
            lens[i] = 0u;
            if (p >= n) continue;
            if ((s.bits >> i) & 1u) {
                ps = p;
                symbols |= 1u << i;
                continue;
            }
            const int k = p - ps - 1, r = ends[i] - ps - 1, q = r / MAXCOPY, rem = r - MAXCOPY * q;
            if (k < MAXCOPY * q) {
                if (k % MAXCOPY == 0) { symbols |= 1u << i; lens[i] = (uint32_t)MAXCOPY; }
            } else if (rem >= 3) {
                if (k == MAXCOPY * q) { symbols |= 1u << i; lens[i] = (uint32_t)rem; }
            } else {
                symbols |= 1u << i;
            }
        }
    }
    const int count = __popc(symbols);
    const int before = block_excl_sum<NT>(count, sh);
    if (!WRITE) {
        if (threadIdx.x == NT - 1) chunks[4 * n_chunks + ch] = before + count;
        return;
    }
    int idx = chunks[4 * n_chunks + ch] + before;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        if (!((symbols >> i) & 1u)) continue;
        if (idx >= 0 && idx < n) tok[im.px_off + idx] = lens[i] ? COPY | lens[i] : s.v[i] & 0xFFFFFFu;      // always: a token covers at least one pixel
        ++idx;
    }
}

__global__ __launch_bounds__(NT) void webp_enc_symscan_kernel(const Image* images, int n_chunks, int32_t* chunks, int64_t* sums) {
    __shared__ int64_t sh[NT];
    const Image im = images[blockIdx.x];
    int32_t* c = chunks + 4 * n_chunks + im.chunk0;
    const int64_t total = scan_by_one_workgroup(c, nullptr, c, im.n_chunks, sh);
    if (threadIdx.x == 0) sums[4 * blockIdx.x] = min(total, (int64_t)im.n_px);
}

// ---- the codes.  prefix_encode of the format: a copy length 1 .. 4096 -> its prefix symbol (0 .. 23), the extra bits and their count
__device__ __forceinline__ void length_prefix(int len, int& sym, int& extra, int& nextra) {
    const int d = len - 1;
    if (d < 4) { sym = d; extra = 0; nextra = 0; return; }
    const int hb = 31 - __clz(d);
    nextra = hb - 1;
    sym = 2 * hb + ((d >> nextra) & 1);
    extra = d & ((1 << nextra) - 1);
}

// green + length (blockIdx.y 0), red (1), blue (2) of one chunk of tokens: a histogram in LDS, its non-zero bins added to the image's
__global__ __launch_bounds__(NT) void webp_enc_hist_kernel(const Image* images, int n_images, const uint32_t* tok, const int64_t* sums, int32_t* hist) {
    __shared__ int h[CW];
    const int ch = blockIdx.x, code = blockIdx.y;
    const int ii = entry_of(n_images, ch, [&](int i) { return images[i].chunk0; });
    const Image im = images[ii];
    const int total = (int)sums[4 * ii];
    const int64_t t0 = (int64_t)(ch - im.chunk0) * CHUNK;
    if (t0 >= total) return;                                                     // the whole workgroup
    for (int i = threadIdx.x; i < CW; i += NT) h[i] = 0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int64_t t = t0 + ITEMS * threadIdx.x + i;
        if (t >= total) continue;
        const uint32_t s = tok[im.px_off + t];
        if (s & COPY) {
            if (code == 0) {
                int sym, extra, nextra;
                length_prefix(min(max((int)(s & 0xFFFFu), 1), MAXCOPY), sym, extra, nextra);
                atomicAdd(&h[256 + sym], 1);
            }
        } else {
            atomicAdd(&h[code == 0 ? (s >> 8) & 255u : code == 1 ? (s >> 16) & 255u : s & 255u], 1);
        }
    }
    __syncthreads();
    int32_t* out = hist + ((int64_t)ii * NCODES + code) * CW;
    for (int i = threadIdx.x; i < CW; i += NT)
        if (h[i]) atomicAdd(out + i, h[i]);
}

__device__ __forceinline__ int alphabet_of(int code) { return code == 0 ? 280 : code == 4 ? 40 : 256; }

// one wave per image and code; the tree is one lane's work (png_trees.h).  codes: length << 16 | the bit-reversed code, per symbol
__global__ __launch_bounds__(64) void webp_enc_codes_kernel(const Image* images, int32_t* hist, int32_t* cinfo, uint32_t* codes, uint32_t* heads) {
    __shared__ png_trees::Work W;
    const int ii = blockIdx.x / NCODES, k = blockIdx.x - NCODES * ii;
    const Image im = images[ii];
    const int alphabet = alphabet_of(k);
    int32_t* hs = hist + ((int64_t)ii * NCODES + k) * CW;
    uint32_t* code = codes + ((int64_t)ii * NCODES + k) * CW;
    uint32_t* head = heads + ((int64_t)ii * NCODES + k) * HW;
    for (int i = threadIdx.x; i < CW; i += 64) code[i] = 0u;
    for (int i = threadIdx.x; i < HW; i += 64) head[i] = 0u;
    if (k >= 3) {                                                                // alpha: every literal has the image's one value; distance: every copy has symbol 1
        const int32_t* green = hist + (int64_t)ii * NCODES * CW;
        int sum = 0;
        for (int i = (k == 3 ? 0 : 256) + threadIdx.x; i < (k == 3 ? 256 : CW); i += 64) sum += green[i];
        for (int d = 32; d; d >>= 1) sum += __shfl_down(sum, d, 64);
        if (threadIdx.x == 0) hs[k == 3 ? im.alpha & 255 : 1] = sum;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < alphabet; i += 64) W.freq[i] = hs[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    int n_used = 0, u0 = 0, u1 = 0;
    for (int i = 0; i < alphabet; ++i) {
        if (W.freq[i] == 0) continue;
        if (n_used == 0) u0 = i;
        u1 = i;
        ++n_used;
    }
    png_trees::HeadWriter hw = {head, HW, 0};
    if (n_used <= 2 && u1 < 256) {                                               // a simple code; nothing used: symbol 0
        const bool first8 = u0 > 1;
        hw.put(1u, 1);
        hw.put(n_used == 2 ? 1u : 0u, 1);
        hw.put(first8 ? 1u : 0u, 1);
        hw.put((uint32_t)u0, first8 ? 8 : 1);
        if (n_used == 2) {
            hw.put((uint32_t)u1, 8);
            code[u0] = 1u << 16;
            code[u1] = (1u << 16) | 1u;
        }
    } else {
        const uint8_t cl_order[png_trees::BL_CODES] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
        png_trees::build_tree(W, png_trees::BLTREE, alphabet, 15);
        for (int n = 0; n < alphabet; ++n) W.llen[n] = (uint8_t)W.len[n];
        png_trees::gen_codes([&](int n) { return (int)W.llen[n]; }, alphabet - 1, [&](int n, uint32_t c, int l) { code[n] = ((uint32_t)l << 16) | c; });
        for (int n = 0; n < png_trees::BL_CODES; ++n) W.freq[n] = 0;
        png_trees::walk_tree(W.llen, alphabet - 1, [&](int sym, int) { W.freq[sym]++; });
        png_trees::build_tree(W, png_trees::BLTREE, png_trees::BL_CODES, 7);
        for (int n = 0; n < png_trees::BL_CODES; ++n) W.bllen[n] = (uint8_t)W.len[n];
        png_trees::gen_codes([&](int n) { return (int)W.bllen[n]; }, png_trees::BL_CODES - 1, [&](int n, uint32_t c, int) { W.blcode[n] = (uint16_t)c; });
        int count = png_trees::BL_CODES;
        for (; count > 4; --count)
            if (W.bllen[cl_order[count - 1]] != 0) break;
        hw.put(0u, 1);
        hw.put((uint32_t)(count - 4), 4);
        for (int i = 0; i < count; ++i) hw.put(W.bllen[cl_order[i]], 3);
        hw.put(0u, 1);                                                           // no max_symbol: the lengths of the whole alphabet follow
        png_trees::walk_tree(W.llen, alphabet - 1, [&](int sym, int n) {
            hw.put(W.blcode[sym], W.bllen[sym]);
            if (sym == 16) hw.put((uint32_t)(n - 3), 2);
            if (sym == 17) hw.put((uint32_t)(n - 3), 3);
            if (sym == 18) hw.put((uint32_t)(n - 11), 7);
        });
    }
    cinfo[8 * ii + k] = min(hw.bits, 32 * HW);
}

// the five code tables of an image in LDS; a token's fields
struct Tables {
    uint32_t code[3 * CW];
    uint32_t alpha, dist;
};

__device__ __forceinline__ void load_tables(Tables& t, const uint32_t* codes, int ii, const Image& im) {
    const uint32_t* c = codes + (int64_t)ii * NCODES * CW;
    for (int i = threadIdx.x; i < 3 * CW; i += NT) t.code[i] = c[i];
    if (threadIdx.x == 0) { t.alpha = c[3 * CW + (im.alpha & 255)]; t.dist = c[4 * CW + 1]; }
    __syncthreads();
}

// the (at most four) fields of a token: value and width, 15 bits at the most each
__device__ __forceinline__ int token_fields(const Tables& t, uint32_t s, uint32_t* val, int* width) {
    if (s & COPY) {
        int sym, extra, nextra;
        length_prefix(min(max((int)(s & 0xFFFFu), 1), MAXCOPY), sym, extra, nextra);
        const uint32_t c = t.code[256 + sym];
        val[0] = c & 0xFFFFu; width[0] = (int)(c >> 16);
        val[1] = (uint32_t)extra; width[1] = nextra;
        val[2] = t.dist & 0xFFFFu; width[2] = (int)(t.dist >> 16);
        val[3] = 0u; width[3] = 0;
    } else {
        const uint32_t g = t.code[(s >> 8) & 255u], r = t.code[CW + ((s >> 16) & 255u)], b = t.code[2 * CW + (s & 255u)];
        val[0] = g & 0xFFFFu; width[0] = (int)(g >> 16);
        val[1] = r & 0xFFFFu; width[1] = (int)(r >> 16);
        val[2] = b & 0xFFFFu; width[2] = (int)(b >> 16);
        val[3] = t.alpha & 0xFFFFu; width[3] = (int)(t.alpha >> 16);
    }
    return width[0] + width[1] + width[2] + width[3];
}

__global__ __launch_bounds__(NT) void webp_enc_tokbits_kernel(const Image* images, int n_images, int n_chunks, const uint32_t* tok, const int64_t* sums,
                                                               const uint32_t* codes, int32_t* chunks) {
    __shared__ Tables T;
    __shared__ int sh_bits;
    const int ch = blockIdx.x;
    const int ii = entry_of(n_images, ch, [&](int i) { return images[i].chunk0; });
    const Image im = images[ii];
    const int total = (int)sums[4 * ii];
    const int64_t t0 = (int64_t)(ch - im.chunk0) * CHUNK;
    if (t0 >= total) {                                                           // the whole workgroup
        if (threadIdx.x == 0) chunks[5 * n_chunks + ch] = 0;
        return;
    }
    if (threadIdx.x == 0) sh_bits = 0;
    load_tables(T, codes, ii, im);
    int bits = 0;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int64_t t = t0 + ITEMS * threadIdx.x + i;
        uint32_t val[4];
        int width[4];
        if (t < total) bits += token_fields(T, tok[im.px_off + t], val, width);
    }
    if (bits) atomicAdd(&sh_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0) chunks[5 * n_chunks + ch] = sh_bits;
}

__global__ __launch_bounds__(NT) void webp_enc_bitscan_kernel(const Image* images, int n_chunks, const int32_t* chunks, int64_t* cbits, const int32_t* cinfo,
                                                               int64_t* sums) {
    __shared__ int64_t sh[NT];
    const Image im = images[blockIdx.x];
    const int64_t total = scan_by_one_workgroup(chunks + 5 * n_chunks + im.chunk0, cbits + im.chunk0, nullptr, im.n_chunks, sh);
    if (threadIdx.x == 0) {
        int64_t head = 0;
        for (int k = 0; k < NCODES; ++k) head += cinfo[8 * blockIdx.x + k];
        sums[4 * blockIdx.x + 1] = head;
        sums[4 * blockIdx.x + 2] = total;
    }
}

// the payload's bytes once the images' first bits are known (sums[4 i + 3])
__device__ __forceinline__ int64_t payload_bytes(const Job& j, const int64_t* sums, int f) {
    const int64_t* m = sums + 4 * (2 * f + 1);
    return min((m[3] + m[1] + m[2] + 7) >> 3, j.packed_bytes);                   // never binds (MAF_WEBP_ENC_BOUND)
}

__global__ __launch_bounds__(NT) void webp_enc_offsets_kernel(const Job* jobs, int n_files, int64_t* sums, int32_t* lengths, int64_t* offsets) {
    __shared__ int64_t sh[NT];
    for (int f = threadIdx.x; f < n_files; f += NT) {
        int64_t* s = sums + 4 * (2 * f);
        s[3] = MAF_WEBP_ENC_LEAD_BITS;
        s[7] = s[3] + s[1] + s[2] + MAF_WEBP_ENC_MAIN_BITS;
        const int64_t payload = payload_bytes(jobs[f], sums, f);
        lengths[f] = (int32_t)(MAF_WEBP_ENC_FILE_BYTES + payload + (payload & 1));
    }
    __syncthreads();
    scan_by_one_workgroup(lengths, offsets, nullptr, n_files, sh);
}

// ors the low bits of `value` (at most 33 significant ones) into the packed words at bit `at`
__device__ __forceinline__ void or_bits(uint32_t* words, int64_t n_words, int64_t at, uint64_t value) {
    const int64_t w = at >> 5;
    const uint64_t x = value << (at & 31);
    if ((uint32_t)x && w >= 0 && w < n_words) atomicOr(words + w, (uint32_t)x);
    if ((uint32_t)(x >> 32) && w >= 0 && w + 1 < n_words) atomicOr(words + w + 1, (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(NT) void webp_enc_emit_kernel(const Job* jobs, const Image* images, int n_images, const uint32_t* tok, const int64_t* sums,
                                                            const int64_t* cbits, const int32_t* cinfo, const uint32_t* codes, const uint32_t* heads, uint8_t* packed) {
    __shared__ Tables T;
    __shared__ int sh[NT];
    const int ch = blockIdx.x;
    const int ii = entry_of(n_images, ch, [&](int i) { return images[i].chunk0; });
    const Image im = images[ii];
    const int total = (int)sums[4 * ii];
    const int64_t t0 = (int64_t)(ch - im.chunk0) * CHUNK;
    if (t0 >= total) return;                                                     // the whole workgroup
    const Job j = jobs[im.file];
    uint32_t* words = reinterpret_cast<uint32_t*>(packed + j.packed_off);
    const int64_t n_words = j.packed_bytes >> 2;
    const int64_t first_bit = sums[4 * ii + 3];
    if (ch == im.chunk0) {                                                       // the descriptions of the five codes, and in front of a file's first image its lead
        int64_t at = first_bit;
        for (int k = 0; k < NCODES; ++k) {
            const int nbits = cinfo[8 * ii + k];
            for (int i = threadIdx.x; 32 * i < nbits && i < HW; i += NT) or_bits(words, n_words, at + 32 * i, heads[((int64_t)ii * NCODES + k) * HW + i]);
            at += nbits;
        }
        if (!im.main && threadIdx.x == 0) {
            const uint64_t lead = 0x2Full | ((uint64_t)(j.w - 1) << 8) | ((uint64_t)(j.h - 1) << 22) | (1ull << 40) | (2ull << 41) | (1ull << 43) |
                                  ((uint64_t)(j.bits - 2) << 46);
            or_bits(words, n_words, 0, lead & 0xFFFFFFFFull);
            or_bits(words, n_words, 32, lead >> 32);
        }
    }
    load_tables(T, codes, ii, im);
    uint32_t val[ITEMS][4];
    int width[ITEMS][4], mine = 0;
#pragma unroll
    for (int e = 0; e < ITEMS; ++e) {
        const int64_t t = t0 + ITEMS * threadIdx.x + e;
#pragma unroll
        for (int q = 0; q < 4; ++q) { val[e][q] = 0u; width[e][q] = 0; }
        if (t < total) mine += token_fields(T, tok[im.px_off + t], val[e], width[e]);
    }
    const int before = block_excl_sum<NT>(mine, sh);
    const int64_t at = first_bit + sums[4 * ii + 1] + cbits[ch] + before;
    int64_t word = at >> 5;
    int fill = (int)(at & 31);
    uint64_t acc = 0;                                                            // the bits gathered for `word`, from bit `fill` of it on
    bool shared = true;                                                          // the first word may hold the end of the thread before
    auto put = [&](uint32_t value, int n) {                                      // n <= 15, fill <= 31
        acc |= (uint64_t)value << fill;
        fill += n;
        if (fill >= 32) {
            if (word >= 0 && word < n_words) {
                if (shared) atomicOr(words + word, (uint32_t)acc); else words[word] = (uint32_t)acc;
            }
            shared = false;
            acc >>= 32;
            fill -= 32;
            ++word;
        }
    };
#pragma unroll
    for (int e = 0; e < ITEMS; ++e)
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (width[e][q]) put(val[e][q], width[e][q]);
    if (fill > 0 && (uint32_t)acc && word >= 0 && word < n_words) atomicOr(words + word, (uint32_t)acc);      // shared with the thread behind
}

// the payload into the file; the chunk that holds the payload's first byte writes the twenty bytes in front of it and the pad byte
__global__ __launch_bounds__(NT) void webp_enc_copy_kernel(const Job* jobs, int n_files, const uint8_t* packed, const int64_t* sums, const int64_t* offsets,
                                                            uint8_t* out, int64_t out_bytes) {
    const int c = blockIdx.x;
    const int f = entry_of(n_files, c, [&](int i) { return jobs[i].copy0; });
    const Job j = jobs[f];
    const int64_t payload = payload_bytes(j, sums, f), first = (int64_t)(c - j.copy0) * MAF_WEBP_ENC_COPY_CHUNK;
    if (first >= payload) return;                                                // the whole workgroup
    const int len = (int)min((int64_t)MAF_WEBP_ENC_COPY_CHUNK, payload - first);
    const uint8_t* src = packed + j.packed_off + first;
    const int64_t o0 = offsets[f] + MAF_WEBP_ENC_FILE_BYTES + first;
    // aligned words of the output (the file starts wherever the one before ended); the words at the chunk's two ends, which it shares with its
    // neighbours or with the frame of the file, byte by byte
    for (int64_t a = (o0 & ~(int64_t)3) + 4 * threadIdx.x; a < o0 + len; a += 4 * NT) {
        const int rel = (int)(a - o0);
        if (rel >= 0 && rel + 4 <= len) {
            if (a + 4 <= out_bytes) *reinterpret_cast<uint32_t*>(out + a) = src[rel] | (src[rel + 1] << 8) | (src[rel + 2] << 16) | ((uint32_t)src[rel + 3] << 24);
        } else {
            for (int i = 0; i < 4; ++i)
                if (rel + i >= 0 && rel + i < len && a + i < out_bytes) out[a + i] = src[rel + i];
        }
    }
    if (first == 0 && threadIdx.x == 0) {
        const int64_t pad = payload & 1;
        const uint32_t riff = (uint32_t)(12 + payload + pad), vp8l = (uint32_t)payload;
        const uint8_t frame[MAF_WEBP_ENC_FILE_BYTES] = {'R', 'I', 'F', 'F', (uint8_t)riff, (uint8_t)(riff >> 8), (uint8_t)(riff >> 16), (uint8_t)(riff >> 24),
                                                        'W', 'E', 'B', 'P', 'V', 'P', '8', 'L', (uint8_t)vp8l, (uint8_t)(vp8l >> 8), (uint8_t)(vp8l >> 16),
                                                        (uint8_t)(vp8l >> 24)};
        const int64_t o = offsets[f];
        for (int i = 0; i < MAF_WEBP_ENC_FILE_BYTES; ++i)
            if (o + i >= 0 && o + i < out_bytes) out[o + i] = frame[i];
        const int64_t at = o + MAF_WEBP_ENC_FILE_BYTES + payload;
        if (pad && at >= 0 && at < out_bytes) out[at] = 0;
    }
}

}  // namespace

extern "C" int maf_webp_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "webp_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_webp_enc_header_t); out[1] = (int32_t)sizeof(maf_webp_enc_job_t); out[2] = (int32_t)sizeof(maf_webp_enc_image_t);
    return 0;
}

extern "C" int maf_webp_encode(const void* blob_host, const void* blob_dev, uint32_t* argb, uint32_t* px, uint32_t* tok, int32_t* modes, int32_t* chunks, int64_t* cbits,
                               int32_t* hist, int64_t* sums, int32_t* cinfo, uint32_t* codes, uint32_t* heads, uint8_t* packed, uint8_t* out, int32_t* lengths,
                               int64_t* offsets, maf_webp_enc_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && argb && px && tok && modes && chunks && cbits && hist && sums && cinfo && codes && heads && packed && out && lengths && offsets,
                "webp_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, argb, px, packed}) && maf_aligned({cbits, sums, offsets}, 8) && maf_aligned({out}, 4),
                "webp_encode: blob, argb, px and packed must be 16-byte aligned, the 64-bit buffers 8-byte aligned, out 4-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_webp_enc_header_t hd = maf_blob_header<maf_webp_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files) && hd.n_images == 2 * hd.n_files, "webp_encode: 1 to 65535 files per call, two images per file");
    MAF_REQUIRE(maf_blob_size_ok(T), "webp_encode: blob size out of range");
    MAF_REQUIRE(hd.n_chunks > 0 && hd.n_chunks < (1 << 30) && hd.n_blocks > 0 && hd.n_blocks < (1 << 30) && hd.n_copy > 0 && hd.n_copy < (1 << 30),
                "webp_encode: chunk or block count out of range");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(Job), T), "webp_encode: the job table lies outside the blob");
    MAF_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(Image), T), "webp_encode: the image table lies outside the blob");
    const Job* jobs = reinterpret_cast<const Job*>(hb + hd.jobs_off);
    const Image* images = reinterpret_cast<const Image*>(hb + hd.images_off);
    int64_t chunk = 0, block = 0, copy = 0, at_px = 0, at_packed = 0, need = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const Job& j = jobs[i];
        MAF_REQUIRE(j.src, "webp_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= MAF_WEBP_ENC_MAX_SIDE && j.h <= MAF_WEBP_ENC_MAX_SIDE, "webp_encode: width and height are 1 to 16384");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "webp_encode: a row pitch below 3 * width");
        MAF_REQUIRE(j.bits >= 2 && j.bits <= 9, "webp_encode: predictor_bits outside 2..9");
        const int64_t bw = (j.w + (1 << j.bits) - 1) >> j.bits, bh = (j.h + (1 << j.bits) - 1) >> j.bits, n = (int64_t)j.w * j.h;
        MAF_REQUIRE(j.bw == bw && j.n_blocks == bw * bh && j.block0 == block, "webp_encode: the files' blocks must follow each other, ceil(w / 2^bits) * ceil(h / 2^bits) each");
        const int64_t bound = MAF_WEBP_ENC_BOUND(n, bw * bh);
        MAF_REQUIRE(j.packed_off == at_packed && (j.packed_bytes & 15) == 0 && j.packed_bytes >= bound,
                    "webp_encode: the packed regions must follow each other, each a multiple of 16 and no smaller than the bound");
        MAF_REQUIRE(j.n_copy == (j.packed_bytes + MAF_WEBP_ENC_COPY_CHUNK - 1) / MAF_WEBP_ENC_COPY_CHUNK && j.copy0 == copy,
                    "webp_encode: the files' copy chunks must follow each other, sized by the bound");
        for (int s = 0; s < 2; ++s) {
            const Image& im = images[2 * i + s];
            MAF_REQUIRE(im.file == i && im.main == s && im.alpha == (s ? 0 : 255) && im.n_px == (s ? n : bw * bh), "webp_encode: a file's images are its sub-image, then its residuals");
            MAF_REQUIRE(im.px_off == at_px && im.chunk0 == chunk && im.n_chunks == (im.n_px + CHUNK - 1) / CHUNK,
                        "webp_encode: the images' regions and chunks must follow each other without gaps");
            at_px += ((int64_t)im.n_px + 3) / 4 * 4;
            chunk += im.n_chunks;
        }
        block += j.n_blocks;
        copy += j.n_copy;
        at_packed += j.packed_bytes;
        need += MAF_WEBP_ENC_FILE_BYTES + bound + 1;
    }
    MAF_REQUIRE(chunk == hd.n_chunks && block == hd.n_blocks && copy == hd.n_copy, "webp_encode: the header's chunk, block or copy count differs from the jobs' sum");
    MAF_REQUIRE(hd.px_words >= at_px && hd.packed_bytes >= at_packed && hd.out_bytes >= need, "webp_encode: a device buffer is smaller than the worst case");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const Job* d_jobs = reinterpret_cast<const Job*>(db + hd.jobs_off);
    const Image* d_images = reinterpret_cast<const Image*>(db + hd.images_off);
    int rc = maf_check_hip(hipMemsetAsync(packed, 0, (size_t)at_packed, s), "webp_encode memset packed");
    if (rc) return rc;
    rc = maf_check_hip(hipMemsetAsync(hist, 0, (size_t)hd.n_images * NCODES * CW * sizeof(int32_t), s), "webp_encode memset hist");
    if (rc) return rc;
    rc = maf_check_hip(hipMemsetAsync(sums, 0, (size_t)hd.n_images * 4 * sizeof(int64_t), s), "webp_encode memset sums");
    if (rc) return rc;
    const dim3 per_chunk(hd.n_chunks), per_image(hd.n_images), block_nt(NT);
    hipLaunchKernelGGL(webp_enc_gather_kernel, per_chunk, block_nt, 0, s, d_jobs, d_images, hd.n_images, argb);
    MAF_LAUNCH_CHECK("webp_enc_gather");
    hipLaunchKernelGGL(webp_enc_modes_kernel, dim3(hd.n_blocks), block_nt, 0, s, d_jobs, d_images, hd.n_files, argb, modes, px);
    MAF_LAUNCH_CHECK("webp_enc_modes");
    hipLaunchKernelGGL(webp_enc_residual_kernel, per_chunk, block_nt, 0, s, d_jobs, d_images, hd.n_images, argb, modes, px);
    MAF_LAUNCH_CHECK("webp_enc_residual");
    hipLaunchKernelGGL(webp_enc_marks_kernel, per_chunk, block_nt, 0, s, d_images, hd.n_images, hd.n_chunks, px, chunks);
    MAF_LAUNCH_CHECK("webp_enc_marks");
    hipLaunchKernelGGL(webp_enc_runs_kernel, per_image, block_nt, 0, s, d_images, hd.n_chunks, chunks);
    MAF_LAUNCH_CHECK("webp_enc_runs");
    hipLaunchKernelGGL(webp_enc_tokens_kernel<false>, per_chunk, block_nt, 0, s, d_images, hd.n_images, hd.n_chunks, px, chunks, tok);
    MAF_LAUNCH_CHECK("webp_enc_tokens (count)");
    hipLaunchKernelGGL(webp_enc_symscan_kernel, per_image, block_nt, 0, s, d_images, hd.n_chunks, chunks, sums);
    MAF_LAUNCH_CHECK("webp_enc_symscan");
    hipLaunchKernelGGL(webp_enc_tokens_kernel<true>, per_chunk, block_nt, 0, s, d_images, hd.n_images, hd.n_chunks, px, chunks, tok);
    MAF_LAUNCH_CHECK("webp_enc_tokens (write)");
    hipLaunchKernelGGL(webp_enc_hist_kernel, dim3(hd.n_chunks, 3), block_nt, 0, s, d_images, hd.n_images, tok, sums, hist);
    MAF_LAUNCH_CHECK("webp_enc_hist");
    hipLaunchKernelGGL(webp_enc_codes_kernel, dim3(hd.n_images * NCODES), dim3(64), 0, s, d_images, hist, cinfo, codes, heads);
    MAF_LAUNCH_CHECK("webp_enc_codes");
    hipLaunchKernelGGL(webp_enc_tokbits_kernel, per_chunk, block_nt, 0, s, d_images, hd.n_images, hd.n_chunks, tok, sums, codes, chunks);
    MAF_LAUNCH_CHECK("webp_enc_tokbits");
    hipLaunchKernelGGL(webp_enc_bitscan_kernel, per_image, block_nt, 0, s, d_images, hd.n_chunks, chunks, cbits, cinfo, sums);
    MAF_LAUNCH_CHECK("webp_enc_bitscan");
    hipLaunchKernelGGL(webp_enc_offsets_kernel, dim3(1), block_nt, 0, s, d_jobs, hd.n_files, sums, lengths, offsets);
    MAF_LAUNCH_CHECK("webp_enc_offsets");
    hipLaunchKernelGGL(webp_enc_emit_kernel, per_chunk, block_nt, 0, s, d_jobs, d_images, hd.n_images, tok, sums, cbits, cinfo, codes, heads, packed);
    MAF_LAUNCH_CHECK("webp_enc_emit");
    hipLaunchKernelGGL(webp_enc_copy_kernel, dim3(hd.n_copy), block_nt, 0, s, d_jobs, hd.n_files, packed, sums, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("webp_enc_copy");
    return 0;
}
