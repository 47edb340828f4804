// Letterbox of decoded uint8 HWC frames into the uint8 NCHW batch the engine takes, and the box rescale back to source pixels
// ("optional GPU letterbox").
//
// Replaces, for a whole batch in one launch each:
//   * letterbox() (yolov6/data/data_augment.py:53-82): cv2.resize(INTER_LINEAR) to new_unpad + copyMakeBorder(BORDER_CONSTANT, color),
//     then precess_image's HWC -> CHW and BGR -> RGB (yolov6/core/inferer.py:169-179) — or datasets.py:277-300 load_image's resize
//     followed by the rect letterbox of __getitem__ (:196-213);
//   * Inferer.rescale (inferer.py:181-195) + .round() (:98).
//
// Pixel rule: OpenCV's uint8 INTER_LINEAR as restated in tests/letterbox_ref.py (the docstring there lists every rule); the kernel equals
// that restatement bit for bit — integer arithmetic, the per-column / per-row coefficients come from the same double -> float sequence.
//   column dx:  fx = float((dx + 0.5) * (1 / (nw / w)) - 0.5), sx = floor(fx), fx -= sx; sx < 0 -> (0, 0); sx >= w - 1 -> (w - 1, 0)
//               a0 = rint((1 - fx) * 2048), a1 = rint(fx * 2048)                     (saturate_cast<short>: round half to even)
//   row dy:     the same sequence, WITHOUT the coefficient clamp (OpenCV clamps only the row index): rows clip(sy), clip(sy + 1)
//   pixel:      S = r[sx] * a0 + r[sx + 1] * a1 (int32);  out = (((S0 >> 4) * b0 >> 16) + ((S1 >> 4) * b1 >> 16) + 2) >> 2, saturated
//   w = 2 nw and h = 2 nh: OpenCV's area-fast path, (a + b + c + d + 2) >> 2;  w = nw and h = nh: a copy
//
// Shape of the letterbox kernel: grid (bands of LB_ROWS output rows, B), one image per grid row.  A workgroup builds the column table of
// its image in LDS once, then per output row stages the source rows it needs (one when the second has weight 0 or is the same row) into LDS with 16-byte loads on the row's
// 16-byte-aligned interior and byte loads on its ragged ends (any pitch, any width: 500 x 3 = 1 500), and writes 4 output pixels per lane
// and plane as one 32-bit store (W is a multiple of 32).  Border rows are pure stores.  Every byte of the output is written exactly once;
// every source read is inside [row * pitch, row * pitch + 3 w) of a row < h.
#include "maf_common.h"
#include "resize_linear.h"

#include <algorithm>

namespace {

constexpr int LB_ROWS = 8;                 // output rows per workgroup
constexpr int LB_MAX_THREADS = 256;

struct LbArgs {
    uint8_t* out;
    const maf_letterbox_image_t* table;    // device table (B > MAF_LETTERBOX_KARG_MAX) or nullptr
    int B, H, W, row_bytes;                // row_bytes: LDS bytes of one staged source row (16-aligned)
    uint32_t color[3];                     // output plane p (R, G, B) -> colour byte replicated 4x
    int src_ch[3];                         // output plane p reads source channel src_ch[p]
    maf_letterbox_image_t img[MAF_LETTERBOX_KARG_MAX];
};

// stage bytes [0, n) of the source row at `src` into lds + (src & 15): aligned 16-byte chunks fully inside the row as one load each,
// the (at most two) partial chunks byte by byte
__device__ __forceinline__ void stage_row(uint8_t* lds, const uint8_t* src, int n, int tid, int nthr) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src);
    const int head = (int)(a & 15);
    const uint8_t* base = src - head;                         // 16-aligned; chunk k covers base + [16k, 16k + 16)
    const int nchunk = (head + n + 15) >> 4;
    for (int k = tid; k < nchunk; k += nthr) {
        const int lo = k * 16, hi = lo + 16;
        if (lo >= head && hi <= head + n) {
            *reinterpret_cast<u32x4_t*>(lds + lo) = *reinterpret_cast<const u32x4_t*>(base + lo);
        } else {
            const int b0 = lo < head ? head : lo, b1 = hi > head + n ? head + n : hi;
            for (int i = b0; i < b1; ++i) lds[i] = base[i];
        }
    }
}

__global__ __launch_bounds__(LB_MAX_THREADS) void letterbox_kernel(const LbArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.y;
    const maf_letterbox_image_t im = a.table ? a.table[b] : a.img[b];
    const int y0 = blockIdx.x * LB_ROWS, y1 = min(y0 + LB_ROWS, a.H);
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int W = a.W, nq = W >> 2;
    uint8_t* out_img = a.out + (size_t)b * 3 * a.H * W;
    const int nw = im.new_w, nh = im.new_h, top = im.top, left = im.left;
    const bool area2 = (im.w == 2 * nw && im.h == 2 * nh);
    const bool copy = (im.w == nw && im.h == nh);
    uint8_t* row0 = lds;
    uint8_t* row1 = lds + a.row_bytes;
    int* tab = reinterpret_cast<int*>(lds + 2 * a.row_bytes);     // [nw] x {3 sx, a0 | a1 << 16}
    const double scx = 1.0 / ((double)nw / (double)im.w), scy = 1.0 / ((double)nh / (double)im.h);

    const bool any_content = y1 > top && y0 < top + nh;
    if (any_content && !area2 && !copy) {
        for (int dx = tid; dx < nw; dx += nthr) {
            int sx; float fx;
            lin_coef(dx, scx, sx, fx);
            if (sx < 0) { sx = 0; fx = 0.f; }
            if (sx >= im.w - 1) { sx = im.w - 1; fx = 0.f; }
            tab[2 * dx] = 3 * sx;
            tab[2 * dx + 1] = (coef_q(1.f - fx) & 0xffff) | (coef_q(fx) << 16);
        }
    }
    const int rb = 3 * im.w;
    for (int y = y0; y < y1; ++y) {
        const int dy = y - top;
        if (dy < 0 || dy >= nh) {                                  // border row: colour only
            for (int q = tid; q < nq; q += nthr)
                for (int p = 0; p < 3; ++p) reinterpret_cast<uint32_t*>(out_img + ((size_t)p * a.H + y) * W)[q] = a.color[p];
            continue;
        }
        int sy0, sy1, b0 = 0, b1 = 0;
        if (area2) {
            sy0 = 2 * dy; sy1 = 2 * dy + 1;
        } else if (copy) {
            sy0 = sy1 = dy;
        } else {
            float fy;
            lin_coef(dy, scy, sy0, fy);
            b0 = coef_q(1.f - fy); b1 = coef_q(fy);
            sy1 = sy0 + 1;
            sy0 = sy0 < 0 ? 0 : (sy0 >= im.h ? im.h - 1 : sy0);
            sy1 = sy1 < 0 ? 0 : (sy1 >= im.h ? im.h - 1 : sy1);
            if (b1 == 0) sy1 = sy0;                                // the second row has weight 0 (a 3x shrink lands on whole rows): not fetched
        }
        const uint8_t* s0 = im.ptr + (size_t)sy0 * im.pitch;
        const uint8_t* s1 = im.ptr + (size_t)sy1 * im.pitch;
        const bool one_row = sy1 == sy0;                           // uniform over the workgroup
        __syncthreads();                                           // the previous row's readers are done with the staging buffers (and the table is built)
        stage_row(row0, s0, rb, tid, nthr);
        if (!one_row) stage_row(row1, s1, rb, tid, nthr);
        __syncthreads();
        const uint8_t* r0 = row0 + (reinterpret_cast<uintptr_t>(s0) & 15);
        const uint8_t* r1 = one_row ? r0 : row1 + (reinterpret_cast<uintptr_t>(s1) & 15);
        for (int q = tid; q < nq; q += nthr) {
            uint32_t v[3] = {0u, 0u, 0u};
            for (int j = 0; j < 4; ++j) {
                const int dx = 4 * q + j - left;
                for (int p = 0; p < 3; ++p) {
                    uint32_t o;
                    if (dx < 0 || dx >= nw) {
                        o = a.color[p] & 0xffu;
                    } else {
                        const int c = a.src_ch[p];
                        if (copy) {                                // equal sizes: the linear rule with a0 = b0 = 2048 is the identity
                            o = r0[3 * dx + c];
                        } else if (area2) {
                            const int i = 6 * dx + c;
                            o = ((int)r0[i] + r0[i + 3] + r1[i] + r1[i + 3] + 2) >> 2;
                        } else {
                            const int xo = tab[2 * dx] + c, co = tab[2 * dx + 1];
                            const int a0 = co & 0xffff, a1 = co >> 16;
                            const int i1 = a1 ? xo + 3 : xo;          // a1 = 0 for the clamped last column: never read past the row
                            const int S0 = r0[xo] * a0 + r0[i1] * a1;
                            int t = (((S0 >> 4) * b0) >> 16) + 2;
                            if (b1) {                              // b1 = 0: the second term is exactly 0
                                const int S1 = r1[xo] * a0 + r1[i1] * a1;
                                t += ((S1 >> 4) * b1) >> 16;
                            }
                            t >>= 2;
                            o = (uint32_t)(t < 0 ? 0 : (t > 255 ? 255 : t));
                        }
                    }
                    v[p] |= o << (8 * j);
                }
            }
            for (int p = 0; p < 3; ++p) reinterpret_cast<uint32_t*>(out_img + ((size_t)p * a.H + y) * W)[q] = v[p];
        }
    }
}

// Inferer.rescale + .round() on the device, in place on the NMS rows: (x - pad) / ratio in fp32 (torch's CPU op order: IEEE divide by the
// fp32 ratio), clamp to the source frame, optional round half to even
__global__ __launch_bounds__(256) void rescale_boxes_kernel(float* rows, const int32_t* count, int max_det, int row_stride, const float* par, int do_round) {
    const int b = blockIdx.x;
    const int n = min(count[b], max_det);
    const float h0 = par[b * 5 + 0], w0 = par[b * 5 + 1], ratio = par[b * 5 + 2], px = par[b * 5 + 3], py = par[b * 5 + 4];
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        float* r = rows + ((size_t)b * max_det + k) * row_stride;
        float x1 = (r[0] - px) / ratio, y1 = (r[1] - py) / ratio, x2 = (r[2] - px) / ratio, y2 = (r[3] - py) / ratio;
        x1 = fminf(fmaxf(x1, 0.f), w0); y1 = fminf(fmaxf(y1, 0.f), h0);
        x2 = fminf(fmaxf(x2, 0.f), w0); y2 = fminf(fmaxf(y2, 0.f), h0);
        if (do_round) { x1 = rintf(x1); y1 = rintf(y1); x2 = rintf(x2); y2 = rintf(y2); }
        r[0] = x1; r[1] = y1; r[2] = x2; r[3] = y2;
    }
}

}  // namespace

extern "C" int64_t maf_letterbox_lds_bytes(const maf_letterbox_image_t* imgs, int32_t B, int32_t W) {
    int max_w = 1;
    for (int i = 0; i < B; ++i) max_w = imgs[i].w > max_w ? imgs[i].w : max_w;
    const int64_t row_bytes = ((int64_t)3 * max_w + 16 + 15) / 16 * 16;
    return 2 * row_bytes + (int64_t)8 * W;
}

extern "C" int maf_letterbox(const maf_letterbox_image_t* imgs, const maf_letterbox_image_t* imgs_dev, int32_t B, int32_t H, int32_t W,
                             const uint8_t* color, int32_t bgr, uint8_t* out, maf_stream_t stream) {
    MAF_REQUIRE(imgs && out && color, "letterbox: null pointer");
    MAF_REQUIRE((reinterpret_cast<uintptr_t>(out) & 3) == 0, "letterbox: out must be 4-byte aligned (32-bit stores)");
    MAF_REQUIRE(B > 0, "letterbox: B must be positive");
    MAF_REQUIRE(B <= MAF_LETTERBOX_KARG_MAX || imgs_dev, "letterbox: more than MAF_LETTERBOX_KARG_MAX images need the device copy of the table (imgs_dev)");
    MAF_REQUIRE(H > 0 && W > 0 && H % 32 == 0 && W % 32 == 0, "letterbox: H and W must be positive multiples of 32");
    for (int i = 0; i < B; ++i) {
        const maf_letterbox_image_t& m = imgs[i];
        MAF_REQUIRE(m.ptr, "letterbox: null frame pointer");
        MAF_REQUIRE(m.h > 0 && m.w > 0 && m.pitch >= 3 * (int64_t)m.w, "letterbox: frame h, w must be positive and the pitch at least 3 w bytes");
        MAF_REQUIRE(m.new_h > 0 && m.new_w > 0 && m.top >= 0 && m.left >= 0, "letterbox: bad unpadded size or offset");
        MAF_REQUIRE(m.top + m.new_h <= H && m.left + m.new_w <= W, "letterbox: the unpadded size plus its offset exceeds the output H x W");
    }
    const int64_t lds = maf_letterbox_lds_bytes(imgs, B, W);
    MAF_REQUIRE(lds <= 64 * 1024, "letterbox: frame width or output width too large for the LDS staging (3 w_max * 2 + 8 W > 64 KiB)");
    LbArgs a = {};
    a.out = out; a.table = B > MAF_LETTERBOX_KARG_MAX ? imgs_dev : nullptr;
    a.B = B; a.H = H; a.W = W;
    a.row_bytes = (int)((lds - (int64_t)8 * W) / 2);
    for (int p = 0; p < 3; ++p) {
        a.src_ch[p] = bgr ? 2 - p : p;
        a.color[p] = 0x01010101u * color[a.src_ch[p]];             // `color` is in the frame's channel order, like copyMakeBorder's value
    }
    if (!a.table)
        for (int i = 0; i < B; ++i) a.img[i] = imgs[i];
    const int threads = std::min(LB_MAX_THREADS, (W / 4 + 63) / 64 * 64);
    hipLaunchKernelGGL(letterbox_kernel, dim3((H + LB_ROWS - 1) / LB_ROWS, B), dim3(threads), (size_t)lds, static_cast<hipStream_t>(stream), a);
    return maf_check_hip(hipGetLastError(), "letterbox launch");
}

extern "C" int maf_rescale_boxes(float* rows, const int32_t* count, int32_t B, int32_t max_det, int32_t row_stride, const float* params,
                                 int32_t do_round, maf_stream_t stream) {
    MAF_REQUIRE(rows && count && params, "rescale_boxes: null pointer");
    MAF_REQUIRE(B > 0 && max_det > 0 && row_stride >= 4, "rescale_boxes: bad shape (B > 0, max_det > 0, row_stride >= 4)");
    hipLaunchKernelGGL(rescale_boxes_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), rows, count, max_det, row_stride, params, do_round ? 1 : 0);
    return maf_check_hip(hipGetLastError(), "rescale_boxes launch");
}
