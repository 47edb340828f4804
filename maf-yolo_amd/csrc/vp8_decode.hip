// Lossy WebP (one VP8 key frame, RFC 6386) decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to libwebp's
// WebPDecodeBGR bit for bit (what cv2.imread (IMREAD_COLOR) asks libwebp for; the argument is in maf-yolo_amd/webp_lossy.py).  Replaces the
// cv2.imread of TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the webp entry of IMG_FORMATS,
// lossy files.  The rules are restated in tests/webp_lossy_ref.py; the per-sample arithmetic is in vp8_rules.h, the constants of the format in
// vp8_tables.h; the host side (RIFF walk, the 10 header bytes, blob) is maf-yolo_amd/webp_lossy.py; blob, buffers and scratch layout are
// described in include/mafyolo_vp8.h.
//
// Four kernels, one launch each for the whole batch:
//   vp8_parse_kernel    A bool-coded partition is one serial chain, so the batch is the parallelism: one one-wave workgroup per image.  Control is
//                       WAVE-UNIFORM: all 64 lanes hold the same reader state, decode the same bool and take the same branch; a value every lane
//                       computes is stored by every lane to the same address.  The lanes differ only where data moves: loading the probability
//                       table, clearing a macroblock's coefficients, the inverse WHT (lane o gives the DC of block o), copying the coefficients
//                       out and finding the non-zero blocks (ballot).  The first partition (frame header, modes) is read in step with the token
//                       partition of the macroblock row (row & (partitions - 1)); the readers of the token partitions rest in LDS between rows.
//                       Coefficients are dequantised as they are read; a macroblock leaves a 32-byte record and 384 int16 coefficients.
//   vp8_recon_kernel    ONE workgroup per image: macroblock (x, y) needs (x - 1, y), (x, y - 1) and (x + 1, y - 1), so a band of 16 macroblock rows
//                       is a staggered wavefront, wave r on row y0 + r two macroblocks behind wave r - 1, one barrier per step.  A wave predicts
//                       and adds the residual in a work tile in LDS (libwebp's layout: the row above with 4 samples above-right, the column to
//                       the left) and stores the macroblock to the unfiltered planes; the left column stays in the tile for the next step, the
//                       row above comes from the planes (the wave above stored it at least one barrier ago).  Inside a 4x4-predicted macroblock
//                       the sub-blocks obey the same rule: ten sub-steps, the (at most two) blocks with bx + 2 by == step side by side, 16 lanes each.
//                       No flags and no spinning between workgroups anywhere.
//   vp8_filter_kernel   ONE workgroup per image: copies the unfiltered planes to yuv and filters there in place, the same lag-2 wavefront (raster
//                       order matters: a macroblock's edges read what its left and upper neighbours left behind).  Per macroblock the left edge
//                       and the inner vertical edges with a lane per row (16 luma, 8 + 8 chroma lanes; a lane keeps its row in registers and
//                       walks the edges left to right), a barrier, then the top edge and the inner horizontal edges with a lane per column.
//   vp8_convert_kernel  One thread per 4 pixels: fancy upsampling, YUV -> BGR, 12 bytes out; zeros for an image whose status is not 0.
//
// Bounded by construction (the parse kernel reads bytes a file controls):
//   * input: every byte index is clamped into the stream section (which ends in zero padding) AND compared with its partition's end, which is
//     at most the image's stream_end; past it the reader feeds zeros and sets MAF_VP8_ST_INPUT_EXHAUSTED (lazily, as libwebp's reader does: only
//     a bool that needs a byte).  Partition sizes from the file are clamped to what is left of the chunk;
//   * stores: every macroblock index is below mbw * mbh of the size the host validated, every coefficient index below 400 (zigzag of n < 16
//     inside one of 25 blocks), modes come out of fixed trees (0 .. 9), the segment is 0 .. 3, quantiser indices are clamped to 0 .. 127,
//     the context arrays in LDS hold 1024 macroblock columns (a side is at most 16383);
//   * loops: the macroblock count, 16 coefficients per block (every pass consumes one), 1056 probabilities, at most 8 partitions, 11 extra
//     bits.  Nothing a file says is a loop bound or an address without such a clamp.
// An image that ends with a non-zero status yields an all-zero frame; RECON and FILTER skip it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "image_blob.h"
#include "vp8_rules.h"
#include "vp8_tables.h"
#include "../../include/mafyolo_vp8.h"

void maf_set_error(const std::string& msg);
int maf_check_hip(hipError_t e, const char* what);
#define VP8_REQUIRE(cond, msg)               \
    do {                                     \
        if (!(cond)) {                       \
            maf_set_error(std::string(msg)); \
            return -1; /* MAF_E_ARG */       \
        }                                    \
    } while (0)

namespace {

constexpr int BAND = 16;                  // macroblock rows of a RECON / FILTER band: one wave each
constexpr int MAX_MBW = 1024;             // macroblock columns of the widest image (16383 samples)
constexpr int WY = 32, WC = 16;           // row pitch of the luma / chroma work tile

struct ScratchLayout {
    int64_t meta, records, coeffs, total;
};
__host__ __device__ inline ScratchLayout scratch_layout(int w, int h) {
    const int64_t n = (int64_t)((w + 15) >> 4) * ((h + 15) >> 4);
    ScratchLayout s;
    s.meta = 0;
    s.records = MAF_VP8_META_WORDS * 4;
    s.coeffs = s.records + n * MAF_VP8_MB_RECORD;
    s.total = s.coeffs + n * MAF_VP8_MB_COEFFS * 2;
    return s;
}

// the lanes of ONE wave: LDS written by some of them is read by others behind this
__device__ inline void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---------------------------------------------------------------- PARSE

struct Input {
    const uint8_t* bytes;                 // the stream section
    int64_t last;                         // its last byte (inside the zero padding)
};

// libwebp's bool reader with byte-wise loads: `range` is kept minus one, `bits` is the count of unread bits minus 8.  A byte is fetched only
// when a bool starts with fewer than 8 unread bits (libwebp fetches 7 at a time where it can; which bool first finds the partition empty does
// not depend on the width of the fetches).
struct BoolReader {
    uint32_t value, range;
    int32_t bits, eof;
    int64_t pos, end;
};
__device__ inline void br_init(BoolReader& b, int64_t begin, int64_t end) {
    b.value = 0; b.range = 254; b.bits = -8; b.eof = 0; b.pos = begin; b.end = end;
}
__device__ inline int br_bit(BoolReader& b, const Input& in, int prob) {
    uint32_t r = b.range;
    if (b.bits < 0) {
        if (b.pos < b.end) {
            b.value = (b.value << 8) | in.bytes[b.pos < in.last ? b.pos : in.last];
            ++b.pos;
            b.bits += 8;
        } else if (!b.eof) {
            b.value <<= 8;
            b.bits += 8;
            b.eof = 1;
        } else {
            b.bits = 0;
        }
    }
    const int pos = b.bits;
    const uint32_t split = (r * (uint32_t)prob) >> 8;
    int bit;
    if ((b.value >> pos) > split) {
        r -= split;
        b.value -= (split + 1) << pos;
        bit = 1;
    } else {
        r = split + 1;
        bit = 0;
    }
    const int shift = 7 ^ (31 - __clz((int)r));
    b.bits -= shift;
    b.range = (r << shift) - 1;
    return bit;
}
__device__ inline int br_value(BoolReader& b, const Input& in, int n) {
    int v = 0;
    while (n-- > 0) v = 2 * v + br_bit(b, in, 128);
    return v;
}
__device__ inline int br_signed(BoolReader& b, const Input& in, int n) {
    const int v = br_value(b, in, n);
    return br_bit(b, in, 128) ? -v : v;
}
__device__ inline int br_opt_signed(BoolReader& b, const Input& in, int n) { return br_bit(b, in, 128) ? br_signed(b, in, n) : 0; }

__device__ inline int large_value(BoolReader& b, const Input& in, const uint8_t* p) {
    if (!br_bit(b, in, p[3])) {
        if (!br_bit(b, in, p[4])) return 2;
        return 3 + br_bit(b, in, p[5]);
    }
    if (!br_bit(b, in, p[6])) {
        if (!br_bit(b, in, p[7])) return 5 + br_bit(b, in, 159);
        const int v = 7 + 2 * br_bit(b, in, 165);
        return v + br_bit(b, in, 145);
    }
    const int bit1 = br_bit(b, in, p[8]);
    const int cat = 2 * bit1 + br_bit(b, in, p[9 + bit1]);
    int v = 0;
    for (int i = 0; i < 11; ++i) {
        const int pr = k_vp8_cat3456[cat][i];
        if (!pr) break;
        v += v + br_bit(b, in, pr);
    }
    return v + 3 + (8 << cat);
}

// The tokens of one block.  P: the probabilities of its type [8 bands][3 contexts][11]; out: the block's 16 coefficients (raster order, zeroed)
// -> one past the last non-zero coefficient in zigzag order.
__device__ inline int get_coeffs(BoolReader& b, const Input& in, const uint8_t* P, int ctx, int dc_q, int ac_q, int n, int16_t* out) {
    const uint8_t* p = P + (k_vp8_bands[n] * 3 + ctx) * 11;
    for (; n < 16; ++n) {
        if (!br_bit(b, in, p[0])) return n;
        while (!br_bit(b, in, p[1])) {
            ++n;
            p = P + k_vp8_bands[n] * 33;
            if (n == 16) return 16;
        }
        const uint8_t* next = P + k_vp8_bands[n + 1] * 33;
        int v;
        if (!br_bit(b, in, p[2])) {
            v = 1;
            p = next + 11;
        } else {
            v = large_value(b, in, p);
            p = next + 22;
        }
        if (br_bit(b, in, 128)) v = -v;
        out[k_vp8_zigzag[n]] = (int16_t)(v * (n > 0 ? ac_q : dc_q));
    }
    return 16;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__global__ __launch_bounds__(64) void vp8_parse_kernel(const maf_vp8_image_t* images, const uint8_t* streams, int64_t stream_bytes, uint8_t* scratch,
                                                        int32_t* status) {
    __shared__ uint8_t proba[4 * 8 * 3 * 11];
    __shared__ uint8_t top_modes[MAX_MBW * 4];
    __shared__ uint16_t top_nz[MAX_MBW];          // bits 0 .. 3 luma columns, 4 5 U, 6 7 V, 8 Y2
    __shared__ BoolReader parts[8];
    __shared__ __attribute__((aligned(16))) int16_t coef[400];     // 24 blocks, then the Y2 block
    __shared__ int32_t quant[4][6];               // per segment: y1 dc ac, y2 dc ac, uv dc ac
    __shared__ uint8_t fstr[4][2][4];             // per segment and 16x16 / 4x4: limit, interior limit, hev threshold
    const int lane = threadIdx.x;
    const maf_vp8_image_t im = images[blockIdx.x];
    const int mbw = (im.w + 15) >> 4, mbh = (im.h + 15) >> 4;
    const ScratchLayout lay = scratch_layout(im.w, im.h);
    uint8_t* sc = scratch + im.scratch_off;
    uint32_t* meta = reinterpret_cast<uint32_t*>(sc + lay.meta);
    uint32_t* records = reinterpret_cast<uint32_t*>(sc + lay.records);
    int16_t* coeffs = reinterpret_cast<int16_t*>(sc + lay.coeffs);
    const Input in{streams, stream_bytes - 1};

    for (int i = lane; i < 1056; i += 64) proba[i] = k_vp8_coeff_proba0[i];
    for (int i = lane; i < mbw * 4; i += 64) top_modes[i] = 0;
    for (int i = lane; i < mbw; i += 64) top_nz[i] = 0;
    __syncthreads();

    int st = 0;
    const int64_t p0_end = im.stream_begin + im.first_part_bytes;
    BoolReader br;
    br_init(br, im.stream_begin, p0_end);
    br_bit(br, in, 128);                           // colour space and clamping type: read and ignored
    br_bit(br, in, 128);
    // segmentation
    int seg_q[4] = {0, 0, 0, 0}, seg_f[4] = {0, 0, 0, 0}, seg_p[3] = {255, 255, 255};
    int update_map = 0, absolute = 0;
    const int use_segment = br_bit(br, in, 128);
    if (use_segment) {
        update_map = br_bit(br, in, 128);
        if (br_bit(br, in, 128)) {
            absolute = br_bit(br, in, 128);
#pragma unroll
            for (int s = 0; s < 4; ++s) seg_q[s] = br_opt_signed(br, in, 7);
#pragma unroll
            for (int s = 0; s < 4; ++s) seg_f[s] = br_opt_signed(br, in, 6);
        }
        if (update_map) {
#pragma unroll
            for (int s = 0; s < 3; ++s) seg_p[s] = br_bit(br, in, 128) ? br_value(br, in, 8) : 255;
        }
    }
    // loop filter
    const int simple = br_bit(br, in, 128);
    const int level = br_value(br, in, 6);
    const int sharpness = br_value(br, in, 3);
    const int use_lf_delta = br_bit(br, in, 128);
    int ref_delta0 = 0, mode_delta0 = 0;
    if (use_lf_delta && br_bit(br, in, 128)) {
        for (int i = 0; i < 8; ++i) {
            if (br_bit(br, in, 128)) {
                const int v = br_signed(br, in, 6);
                if (i == 0) ref_delta0 = v;        // a key frame uses the intra-frame reference delta and the 4x4 mode delta only
                if (i == 4) mode_delta0 = v;
            }
        }
    }
    const int filter_type = level == 0 ? 0 : simple ? 1 : 2;
    // token partitions
    const int nparts = 1 << br_value(br, in, 2);
    {
        int64_t start = p0_end + 3 * (nparts - 1);
        if (start > im.stream_end) {
            st |= MAF_VP8_ST_BAD_PARTITIONS;
        } else {
            for (int p = 0; p < nparts - 1; ++p) {
                int64_t size = 0;
                for (int k = 0; k < 3; ++k) {
                    const int64_t at = p0_end + 3 * p + k;
                    size |= (int64_t)in.bytes[at < in.last ? at : in.last] << (8 * k);
                }
                const int64_t left = im.stream_end - start;
                size = size > left ? left : size;
                if (lane == 0) br_init(parts[p], start, start + size);
                start += size;
            }
            if (lane == 0) br_init(parts[nparts - 1], start, im.stream_end);
            if (start >= im.stream_end) st |= MAF_VP8_ST_BAD_PARTITIONS;
        }
    }
    if (st) {                                      // wave-uniform
        if (lane == 0) {
            status[blockIdx.x] = st;
            meta[0] = 0;
        }
        return;
    }
    // quantisers
    const int base_q = br_value(br, in, 7);
    int dq[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) dq[i] = br_opt_signed(br, in, 4);       // y1 dc, y2 dc, y2 ac, uv dc, uv ac
    if (lane < 4) {
        int sq = 0, sf = 0;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s == lane) {
                sq = seg_q[s];
                sf = seg_f[s];
            }
        }
        const int q = use_segment ? sq + (absolute ? 0 : base_q) : base_q;
        quant[lane][0] = k_vp8_dc_q[clampi(q + dq[0], 0, 127)];
        quant[lane][1] = k_vp8_ac_q[clampi(q, 0, 127)];
        quant[lane][2] = k_vp8_dc_q[clampi(q + dq[1], 0, 127)] * 2;
        const int y2ac = (k_vp8_ac_q[clampi(q + dq[2], 0, 127)] * 101581) >> 16;
        quant[lane][3] = y2ac < 8 ? 8 : y2ac;
        quant[lane][4] = k_vp8_dc_q[clampi(q + dq[3], 0, 117)];
        quant[lane][5] = k_vp8_ac_q[clampi(q + dq[4], 0, 127)];
        const int base_level = use_segment ? sf + (absolute ? 0 : level) : level;
        for (int i4 = 0; i4 < 2; ++i4) {
            int lv = base_level;
            if (use_lf_delta) lv += ref_delta0 + (i4 ? mode_delta0 : 0);
            lv = clampi(lv, 0, 63);
            int limit = 0, il = 0, hev = 0;
            if (lv > 0) {
                il = lv;
                if (sharpness > 0) {
                    il >>= sharpness > 4 ? 2 : 1;
                    if (il > 9 - sharpness) il = 9 - sharpness;
                }
                if (il < 1) il = 1;
                limit = 2 * lv + il;
                hev = lv >= 40 ? 2 : lv >= 15 ? 1 : 0;
            }
            fstr[lane][i4][0] = (uint8_t)limit;
            fstr[lane][i4][1] = (uint8_t)il;
            fstr[lane][i4][2] = (uint8_t)hev;
        }
    }
    br_bit(br, in, 128);                           // refresh of the entropy probabilities: read and ignored
    for (int i = 0; i < 1056; ++i) {
        if (br_bit(br, in, k_vp8_coeff_update[i])) proba[i] = (uint8_t)br_value(br, in, 8);   // every lane stores the same value
    }
    const int use_skip = br_bit(br, in, 128);
    const int skip_p = use_skip ? br_value(br, in, 8) : 0;
    __syncthreads();                               // parts, quant, fstr, proba

    BoolReader tr = parts[0];
    int cur = 0;
    for (int my = 0; my < mbh; ++my) {
        const int want = my & (nparts - 1);
        if (want != cur) {
            if (lane == 0) parts[cur] = tr;
            wave_sync();
            tr = parts[want];
            cur = want;
        }
        uint32_t left_modes = 0, left_nz = 0;      // 4 sub-modes (a byte each); the bits of top_nz
        for (int mx = 0; mx < mbw; ++mx) {
            const int64_t mb = (int64_t)my * mbw + mx;
            for (int i = lane; i < 200; i += 64) reinterpret_cast<uint32_t*>(coef)[i] = 0;
            wave_sync();
            // ---- modes (first partition)
            int segment = 0;
            if (update_map) segment = !br_bit(br, in, seg_p[0]) ? br_bit(br, in, seg_p[1]) : 2 + br_bit(br, in, seg_p[2]);
            const int skip = use_skip ? br_bit(br, in, skip_p) : 0;
            const int i4 = !br_bit(br, in, 145);
            int ymode = 0;
            uint32_t modes[4] = {0, 0, 0, 0};      // row y of the sub-modes, a byte each
            uint32_t tm = *reinterpret_cast<const uint32_t*>(top_modes + 4 * mx);
            if (!i4) {
                ymode = br_bit(br, in, 156) ? (br_bit(br, in, 128) ? 1 : 3) : (br_bit(br, in, 163) ? 2 : 0);
                tm = left_modes = (uint32_t)ymode * 0x01010101u;
            } else {
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    int m = (left_modes >> (8 * y)) & 255;
#pragma unroll
                    for (int x = 0; x < 4; ++x) {
                        const uint8_t* p = k_vp8_bmode_proba + ((((tm >> (8 * x)) & 255) * 10) + m) * 9;
                        m = !br_bit(br, in, p[0]) ? 0
                            : !br_bit(br, in, p[1]) ? 1
                            : !br_bit(br, in, p[2]) ? 2
                            : !br_bit(br, in, p[3]) ? (!br_bit(br, in, p[4]) ? 3 : (!br_bit(br, in, p[5]) ? 4 : 5))
                                                    : (!br_bit(br, in, p[6]) ? 6 : (!br_bit(br, in, p[7]) ? 7 : (!br_bit(br, in, p[8]) ? 8 : 9)));
                        tm = (tm & ~(255u << (8 * x))) | ((uint32_t)m << (8 * x));
                    }
                    modes[y] = tm;
                    left_modes = (left_modes & ~(255u << (8 * y))) | ((uint32_t)m << (8 * y));
                }
            }
            *reinterpret_cast<uint32_t*>(top_modes + 4 * mx) = tm;
            const int uvmode = !br_bit(br, in, 142) ? 0 : !br_bit(br, in, 114) ? 2 : br_bit(br, in, 183) ? 1 : 3;
            // ---- tokens (the row's partition)
            uint32_t tnz = top_nz[mx], lnz = left_nz;
            int nz_y2 = 0;
            if (!skip) {
                const int32_t* q = quant[segment];
                int first = 0, type = 3;
                if (!i4) {
                    nz_y2 = get_coeffs(tr, in, proba + 264, ((tnz >> 8) & 1) + ((lnz >> 8) & 1), q[2], q[3], 0, coef + 384);
                    const uint32_t f = nz_y2 > 0;
                    tnz = (tnz & ~256u) | (f << 8);
                    lnz = (lnz & ~256u) | (f << 8);
                    first = 1;
                    type = 0;
                }
                for (int y = 0; y < 4; ++y) {
                    for (int x = 0; x < 4; ++x) {
                        const int nz = get_coeffs(tr, in, proba + type * 264, ((tnz >> x) & 1) + ((lnz >> y) & 1), q[0], q[1], first, coef + (4 * y + x) * 16);
                        const uint32_t f = nz > first;
                        tnz = (tnz & ~(1u << x)) | (f << x);
                        lnz = (lnz & ~(1u << y)) | (f << y);
                    }
                }
                for (int ch = 0; ch < 2; ++ch) {
                    for (int y = 0; y < 2; ++y) {
                        for (int x = 0; x < 2; ++x) {
                            const int bt = 4 + 2 * ch + x, bl = 4 + 2 * ch + y;
                            const int nz = get_coeffs(tr, in, proba + 2 * 264, ((tnz >> bt) & 1) + ((lnz >> bl) & 1), q[4], q[5], 0,
                                                      coef + (16 + 4 * ch + 2 * y + x) * 16);
                            const uint32_t f = nz > 0;
                            tnz = (tnz & ~(1u << bt)) | (f << bt);
                            lnz = (lnz & ~(1u << bl)) | (f << bl);
                        }
                    }
                }
            } else {                               // nothing coded: the contexts are cleared, the Y2 one only if this macroblock has a Y2 block
                tnz = i4 ? (tnz & 256u) : 0;
                lnz = i4 ? (lnz & 256u) : 0;
            }
            top_nz[mx] = (uint16_t)tnz;
            left_nz = lnz;
            wave_sync();
            // ---- the Y2 block becomes the DC of the 16 luma blocks
            if (!i4 && !skip) {
                if (lane < 16) {
                    const int dc = nz_y2 > 1 ? vp8_iwht(coef + 384, lane) : ((int)coef[384] + 3) >> 3;
                    coef[lane * 16] = (int16_t)dc;
                }
                wave_sync();
            }
            // ---- out: the coefficients, the mask of non-zero blocks, the record
            uint32_t mask = 0;
            uint32_t* dst = reinterpret_cast<uint32_t*>(coeffs + mb * MAF_VP8_MB_COEFFS);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const uint32_t wv = reinterpret_cast<const uint32_t*>(coef)[lane + 64 * k];
                dst[lane + 64 * k] = wv;
                const uint64_t bal = __ballot(wv != 0);
                for (int b = 0; b < 8; ++b)
                    if ((bal >> (8 * b)) & 255) mask |= 1u << (8 * k + b);
            }
            if (lane == 0) {
                const uint8_t* fs = fstr[segment][i4];
                const uint32_t inner = i4 || mask != 0;
                uint32_t* rec = records + mb * (MAF_VP8_MB_RECORD / 4);
                rec[0] = (uint32_t)i4 | (inner << 1) | ((uint32_t)skip << 2) | ((uint32_t)ymode << 8) | ((uint32_t)uvmode << 16) | ((uint32_t)fs[0] << 24);
                rec[1] = (uint32_t)fs[1] | ((uint32_t)fs[2] << 8);
                rec[2] = modes[0]; rec[3] = modes[1]; rec[4] = modes[2]; rec[5] = modes[3];
                rec[6] = mask;
                rec[7] = 0;
            }
            wave_sync();                           // the copy read coef: the next macroblock clears it
        }
    }
    if (lane == 0) parts[cur] = tr;
    wave_sync();
    int eof = br.eof;
    for (int p = 0; p < nparts; ++p) eof |= parts[p].eof;
    if (eof) st |= MAF_VP8_ST_INPUT_EXHAUSTED;
    if (lane == 0) {
        status[blockIdx.x] = st;
        meta[0] = (uint32_t)filter_type;
    }
}

// ---------------------------------------------------------------- RECON

struct Planes {
    uint8_t *y, *u, *v;
    int64_t ys, cs;                        // row pitch of luma / chroma
};
__device__ inline Planes planes_of(uint8_t* base, const maf_vp8_image_t& im) {
    const int mbw = (im.w + 15) >> 4, mbh = (im.h + 15) >> 4;
    const int64_t n = (int64_t)mbw * mbh;
    Planes p;
    p.y = base + im.planes_off;
    p.u = p.y + 256 * n;
    p.v = p.u + 64 * n;
    p.ys = 16 * (int64_t)mbw;
    p.cs = 8 * (int64_t)mbw;
    return p;
}

// The row above (with `extra` samples above-right) and, in the first column, the column to the left of an N x N block of plane P, with the
// normative borders, into the work tile W (pitch WP; W[0] is the corner).  Lanes first .. first + N + extra.
template <int N, int WP>
__device__ inline void load_context(uint8_t* W, const uint8_t* P, int64_t pitch, int mx, int my, int mbw, int extra, int k) {
    if (k < 0 || k > N + extra) return;
    const int c = k - 1;                                               // -1 .. N + extra - 1
    int v = 127;
    if (my > 0) {
        const uint8_t* above = P + ((int64_t)N * my - 1) * pitch + (int64_t)N * mx;
        if (c < 0) v = mx ? above[-1] : 129;
        else if (c < N) v = above[c];
        else v = mx == mbw - 1 ? above[N - 1] : above[c];
    }
    W[k] = (uint8_t)v;
}

// N x N prediction (16x16 luma or 8x8 chroma) of the 4 samples of row `row` from column col0, then the residual of block row i
template <int N, int WP>
__device__ inline void predict_add(uint8_t* W, int mode, int mx, int my, int row, int col0, const int16_t* co, bool nonzero, int i) {
    int dc = 128;
    if (mode == 0) {
        int st = 0, sl = 0;
        for (int k = 0; k < N; ++k) {
            st += W[1 + k];
            sl += W[(k + 1) * WP];
        }
        constexpr int SH = N == 16 ? 4 : 3;
        if (mx && my) dc = (st + sl + N) >> (SH + 1);
        else if (my) dc = (st + (N >> 1)) >> SH;
        else if (mx) dc = (sl + (N >> 1)) >> SH;
    }
    const int corner = W[0], left = W[(row + 1) * WP];
    int r[4] = {0, 0, 0, 0};
    if (nonzero) vp8_idct_row(co, i, r);
    int out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int top = W[1 + col0 + k];
        const int p = mode == 0 ? dc : mode == 1 ? vp8_clip255(top + left - corner) : mode == 2 ? top : left;
        out[k] = vp8_clip255(p + r[k]);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) W[(row + 1) * WP + 1 + col0 + k] = (uint8_t)out[k];
}

__device__ inline void recon_mb(uint8_t* W, uint8_t* WU, uint8_t* WV, const Planes& pl, const uint32_t* rec, const int16_t* co, int mx, int my, int mbw,
                                int lane) {
    const uint32_t w0 = rec[0], mask = rec[6];
    const int i4 = w0 & 1, ymode = (w0 >> 8) & 255, uvmode = (w0 >> 16) & 255;
    // the context: the row above from the planes; in the first column the left border (else the previous step left it in the tile)
    load_context<16, WY>(W, pl.y, pl.ys, mx, my, mbw, 4, lane);
    load_context<8, WC>(WU, pl.u, pl.cs, mx, my, mbw, 0, lane - 24);
    load_context<8, WC>(WV, pl.v, pl.cs, mx, my, mbw, 0, lane - 36);
    if (mx == 0 && lane >= 48) {
        const int r = lane - 48;
        W[(r + 1) * WY] = 129;
        if (r < 8) WU[(r + 1) * WC] = WV[(r + 1) * WC] = 129;
    }
    wave_sync();
    if (i4) {
        if (lane < 12) W[4 * ((lane >> 2) + 1) * WY + 17 + (lane & 3)] = W[17 + (lane & 3)];    // above-right of rows 1 to 3 of column 3: that of row 0
        wave_sync();
        const int g = lane >> 4, idx = lane & 15, px = idx & 3, py = idx >> 2;
        for (int s = 0; s < 10; ++s) {
            const int by = (s < 4 ? 0 : (s - 2) >> 1) + g, bx = s - 2 * by;
            const bool active = g < 2 && by <= 3 && bx >= 0 && bx <= 3;
            int val = 0;
            if (active) {
                const int b = 4 * by + bx;
                const int mode = (rec[2 + by] >> (8 * bx)) & 255;
                const uint8_t* above = W + 4 * by * WY + 4 * bx;       // the corner of this block
                int e[13];
#pragma unroll
                for (int k = 0; k < 4; ++k) e[k] = above[(4 - k) * WY];
#pragma unroll
                for (int k = 0; k < 9; ++k) e[4 + k] = above[k];
                val = vp8_pred4(mode, e, px, py);
                if ((mask >> b) & 1) {
                    int r[4];
                    vp8_idct_row(co + 16 * b, py, r);
                    val = vp8_clip255(val + (px == 0 ? r[0] : px == 1 ? r[1] : px == 2 ? r[2] : r[3]));
                }
            }
            wave_sync();
            if (active) W[(4 * by + py + 1) * WY + 4 * bx + px + 1] = (uint8_t)val;
            wave_sync();
        }
    } else {
        const int b = lane >> 2, i = lane & 3;
        predict_add<16, WY>(W, ymode, mx, my, (b >> 2) * 4 + i, (b & 3) * 4, co + 16 * b, (mask >> b) & 1, i);
    }
    if (lane < 32) {
        const int ch = lane >> 4, b = (lane >> 2) & 3, i = lane & 3;
        predict_add<8, WC>(ch ? WV : WU, uvmode, mx, my, (b >> 1) * 4 + i, (b & 1) * 4, co + 16 * (16 + 4 * ch + b), (mask >> (16 + 4 * ch + b)) & 1, i);
    }
    wave_sync();
    {   // the macroblock goes to the planes, 4 samples per store
        const int row = lane >> 2, c0 = (lane & 3) * 4;
        const uint8_t* s = W + (row + 1) * WY + 1 + c0;
        *reinterpret_cast<uint32_t*>(pl.y + (16 * (int64_t)my + row) * pl.ys + 16 * (int64_t)mx + c0) = s[0] | (s[1] << 8) | (s[2] << 16) | ((uint32_t)s[3] << 24);
        if (lane < 32) {
            const int ch = lane >> 4, r = (lane >> 1) & 7, cc = (lane & 1) * 4;
            const uint8_t* t = (ch ? WV : WU) + (r + 1) * WC + 1 + cc;
            *reinterpret_cast<uint32_t*>((ch ? pl.v : pl.u) + (8 * (int64_t)my + r) * pl.cs + 8 * (int64_t)mx + cc) =
                t[0] | (t[1] << 8) | (t[2] << 16) | ((uint32_t)t[3] << 24);
        }
    }
    // the last column becomes the left column of the next macroblock of this row
    if (lane < 16) W[(lane + 1) * WY] = W[(lane + 1) * WY + 16];
    else if (lane < 32) {
        uint8_t* T = lane < 24 ? WU : WV;
        const int r = lane & 7;
        T[(r + 1) * WC] = T[(r + 1) * WC + 8];
    }
    wave_sync();
}

__global__ __launch_bounds__(64 * BAND) void vp8_recon_kernel(const maf_vp8_image_t* images, const uint8_t* scratch, uint8_t* recon, const int32_t* status) {
    __shared__ uint8_t wy[BAND][17 * WY];
    __shared__ uint8_t wc[BAND][2][9 * WC];
    if (status[blockIdx.x] != 0) return;                       // the whole workgroup
    const maf_vp8_image_t im = images[blockIdx.x];
    const int mbw = (im.w + 15) >> 4, mbh = (im.h + 15) >> 4;
    const ScratchLayout lay = scratch_layout(im.w, im.h);
    const uint8_t* sc = scratch + im.scratch_off;
    const uint32_t* records = reinterpret_cast<const uint32_t*>(sc + lay.records);
    const int16_t* coeffs = reinterpret_cast<const int16_t*>(sc + lay.coeffs);
    const Planes pl = planes_of(recon, im);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int y0 = 0; y0 < mbh; y0 += BAND) {
        const int rows = min(BAND, mbh - y0), steps = mbw + 2 * (rows - 1);
        const int my = y0 + wave;
        for (int t = 0; t < steps; ++t) {                      // the same count for every wave: the barrier below is reached by all
            const int mx = t - 2 * wave;
            if (wave < rows && mx >= 0 && mx < mbw) {
                const int64_t mb = (int64_t)my * mbw + mx;
                recon_mb(wy[wave], wc[wave][0], wc[wave][1], pl, records + mb * (MAF_VP8_MB_RECORD / 4), coeffs + mb * MAF_VP8_MB_COEFFS, mx, my, mbw, lane);
            }
            __threadfence_block();
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------- FILTER

// One line of N samples of a macroblock across its edges (p: its first sample, step: the distance of neighbours across the edges), with the 4
// samples in front of it where the macroblock has a neighbour there: the macroblock edge, then the inner edges in order.
template <int N>
__device__ inline void filter_line(uint8_t* p, int64_t step, bool mb_edge, bool inner, bool simple, int limit, int ilevel, int hev) {
    int s[N + 4];
#pragma unroll
    for (int k = 0; k < N + 4; ++k) s[k] = (k >= 4 || mb_edge) ? p[(k - 4) * step] : 0;
    if (mb_edge) {
        if (simple) vp8_simple_filter(s, limit + 4);
        else vp8_normal_filter(s, limit + 4, ilevel, hev, true);
    }
    if (inner) {
#pragma unroll
        for (int e = 4; e < N; e += 4) {
            if (simple) vp8_simple_filter(s + e, limit);
            else vp8_normal_filter(s + e, limit, ilevel, hev, false);
        }
    }
#pragma unroll
    for (int k = 0; k < N + 4; ++k)
        if (k >= 4 || mb_edge) p[(k - 4) * step] = (uint8_t)s[k];
}

// phase 0: the edges between columns (a lane per row), phase 1: the edges between rows (a lane per column)
__device__ inline void filter_mb(const Planes& pl, const uint32_t* rec, int ftype, int mx, int my, int lane, int phase) {
    const uint32_t w0 = rec[0], w1 = rec[1];
    const int limit = w0 >> 24, ilevel = w1 & 255, hev = (w1 >> 8) & 255;
    const bool inner = (w0 >> 1) & 1, simple = ftype == 1;
    if (limit == 0 || lane >= 32 || (simple && lane >= 16)) return;
    const bool mb_edge = phase == 0 ? mx > 0 : my > 0;
    if (lane < 16) {
        uint8_t* p = pl.y + 16 * (int64_t)my * pl.ys + 16 * (int64_t)mx + (phase == 0 ? lane * pl.ys : lane);
        filter_line<16>(p, phase == 0 ? 1 : pl.ys, mb_edge, inner, simple, limit, ilevel, hev);
    } else {
        const int k = lane & 7;
        uint8_t* p = (lane < 24 ? pl.u : pl.v) + 8 * (int64_t)my * pl.cs + 8 * (int64_t)mx + (phase == 0 ? k * pl.cs : k);
        filter_line<8>(p, phase == 0 ? 1 : pl.cs, mb_edge, inner, false, limit, ilevel, hev);
    }
}

__global__ __launch_bounds__(64 * BAND) void vp8_filter_kernel(const maf_vp8_image_t* images, const uint8_t* scratch, const uint8_t* recon, uint8_t* yuv,
                                                                const int32_t* status) {
    if (status[blockIdx.x] != 0) return;                       // the whole workgroup
    const maf_vp8_image_t im = images[blockIdx.x];
    const int mbw = (im.w + 15) >> 4, mbh = (im.h + 15) >> 4;
    const ScratchLayout lay = scratch_layout(im.w, im.h);
    const uint8_t* sc = scratch + im.scratch_off;
    const uint32_t* records = reinterpret_cast<const uint32_t*>(sc + lay.records);
    const int64_t quads = (int64_t)mbw * mbh * 24;             // 384 bytes per macroblock, 16 at a time
    const uint4* src = reinterpret_cast<const uint4*>(recon + im.planes_off);
    uint4* dst = reinterpret_cast<uint4*>(yuv + im.planes_off);
    for (int64_t i = threadIdx.x; i < quads; i += blockDim.x) dst[i] = src[i];
    __threadfence_block();
    __syncthreads();
    const int ftype = (int)reinterpret_cast<const uint32_t*>(sc + lay.meta)[0];
    if (ftype == 0) return;                                    // the whole workgroup
    const Planes pl = planes_of(yuv, im);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int y0 = 0; y0 < mbh; y0 += BAND) {
        const int rows = min(BAND, mbh - y0), steps = mbw + 2 * (rows - 1);
        const int my = y0 + wave;
        for (int t = 0; t < steps; ++t) {
            const int mx = t - 2 * wave;
            const bool active = wave < rows && mx >= 0 && mx < mbw;
            const uint32_t* rec = records + ((int64_t)my * mbw + mx) * (MAF_VP8_MB_RECORD / 4);
            for (int phase = 0; phase < 2; ++phase) {
                if (active) filter_mb(pl, rec, ftype, mx, my, lane, phase);
                __threadfence_block();
                __syncthreads();
            }
        }
    }
}

// ---------------------------------------------------------------- CONVERT

__global__ __launch_bounds__(256) void vp8_convert_kernel(const maf_vp8_image_t* images, const uint8_t* yuv, uint8_t* out, const int32_t* status) {
    const maf_vp8_image_t im = images[blockIdx.y];
    const int64_t npix = (int64_t)im.w * im.h;
    const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;   // the grid is sized by the largest image of the call
    if (q >= npix) return;
    const bool bad = status[blockIdx.y] != 0;
    const Planes pl = planes_of(const_cast<uint8_t*>(yuv), im);
    const int cw = (im.w + 1) >> 1, ch = (im.h + 1) >> 1;
    const int n = (int)min((int64_t)4, npix - q);
    uint8_t px[12];
    for (int j = 0; j < 4; ++j) {
        px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = 0;
        if (j < n && !bad) {
            const int r = (int)((q + j) / im.w), c = (int)((q + j) % im.w);
            int nr, fr, nc, fc;
            vp8_chroma_pair(r, ch, &nr, &fr);
            vp8_chroma_pair(c, cw, &nc, &fc);
            const int64_t a = nr * pl.cs, b = fr * pl.cs;
            const int u = vp8_upsample(pl.u[a + nc], pl.u[a + fc], pl.u[b + nc], pl.u[b + fc]);
            const int v = vp8_upsample(pl.v[a + nc], pl.v[a + fc], pl.v[b + nc], pl.v[b + fc]);
            vp8_yuv_to_bgr(pl.y[r * pl.ys + c], u, v, px + 3 * j);
        }
    }
    const int64_t o = im.out_off + 3 * q;                      // a multiple of 4: out_off is one of 16 and q one of 4
    if (n == 4) {
        uint32_t* d = reinterpret_cast<uint32_t*>(out + o);
        for (int k = 0; k < 3; ++k) d[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) out[o + k] = px[k];
    }
}

}  // namespace

extern "C" int maf_vp8_struct_sizes(int32_t* out) {
    VP8_REQUIRE(out, "vp8_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_vp8_header_t); out[1] = (int32_t)sizeof(maf_vp8_image_t);
    return 0;
}

extern "C" int maf_vp8_decode(const void* blob_host, const void* blob_dev, uint8_t* scratch, uint8_t* recon, uint8_t* yuv, uint8_t* out, int32_t* status,
                              int32_t stages, maf_vp8_stream_t stream) {
    VP8_REQUIRE(blob_host && blob_dev && scratch && recon && yuv && out && status, "vp8_decode: null pointer");
    VP8_REQUIRE(stages > 0 && (stages & ~MAF_VP8_STAGE_ALL) == 0, "vp8_decode: stages is a mask of MAF_VP8_STAGE_*");
    VP8_REQUIRE(maf_aligned({blob_dev, scratch, recon, yuv, out}), "vp8_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_vp8_header_t hd = maf_blob_header<maf_vp8_header_t>(hb);
    const int64_t T = hd.total_bytes;
    VP8_REQUIRE(maf_blob_count_ok(hd.n_images), "vp8_decode: 1 to 65535 images per call");
    VP8_REQUIRE(maf_blob_size_ok(T), "vp8_decode: blob size out of range");
    VP8_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_vp8_image_t), T) && in_blob(hd.stream_off, hd.stream_bytes, T) &&
                hd.stream_bytes >= MAF_VP8_STREAM_PAD, "vp8_decode: a blob section lies outside the blob");
    VP8_REQUIRE(hd.scratch_bytes > 0 && hd.plane_bytes > 0 && hd.out_bytes > 0, "vp8_decode: empty output buffers");
    const maf_vp8_image_t* ims = reinterpret_cast<const maf_vp8_image_t*>(hb + hd.images_off);
    const int64_t stream_data = hd.stream_bytes - MAF_VP8_STREAM_PAD;
    int64_t max_quads = 1;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_vp8_image_t& m = ims[i];
        VP8_REQUIRE(m.w > 0 && m.h > 0 && m.w <= MAF_VP8_MAX_SIDE && m.h <= MAF_VP8_MAX_SIDE, "vp8_decode: bad image size");
        const int64_t px = (int64_t)m.w * m.h;
        const int64_t mbs = (int64_t)((m.w + 15) >> 4) * ((m.h + 15) >> 4);
        VP8_REQUIRE(3 * px < ((int64_t)1 << 31) && 768 * mbs < ((int64_t)1 << 31), "vp8_decode: an image of 2 GiB or more");
        VP8_REQUIRE(m.stream_begin >= 0 && m.stream_begin <= m.stream_end && m.stream_end <= stream_data, "vp8_decode: an image's stream lies outside the stream section");
        VP8_REQUIRE(m.first_part_bytes >= 0 && m.first_part_bytes <= m.stream_end - m.stream_begin, "vp8_decode: a first partition that runs past its chunk");
        const ScratchLayout lay = scratch_layout(m.w, m.h);
        VP8_REQUIRE(m.scratch_off >= 0 && m.scratch_off % 16 == 0 && m.scratch_bytes >= lay.total && m.scratch_off <= hd.scratch_bytes &&
                    m.scratch_bytes <= hd.scratch_bytes - m.scratch_off, "vp8_decode: an image's scratch lies outside the scratch buffer");
        VP8_REQUIRE(m.planes_off >= 0 && m.planes_off % 16 == 0 && m.planes_off <= hd.plane_bytes && 384 * mbs <= hd.plane_bytes - m.planes_off,
                    "vp8_decode: an image's planes lie outside the plane buffers");
        VP8_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off <= hd.out_bytes && 3 * px <= hd.out_bytes - m.out_off,
                    "vp8_decode: a frame lies outside the output buffer");
        const int64_t quads = (px + 3) / 4;
        max_quads = quads > max_quads ? quads : max_quads;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_vp8_image_t* d_ims = reinterpret_cast<const maf_vp8_image_t*>(db + hd.images_off);
    if (stages & MAF_VP8_STAGE_PARSE) {
        hipLaunchKernelGGL(vp8_parse_kernel, dim3(hd.n_images), dim3(64), 0, s, d_ims, db + hd.stream_off, hd.stream_bytes, scratch, status);
        const int rl = maf_check_hip(hipGetLastError(), "vp8_parse launch");
        if (rl) return rl;
    }
    if (stages & MAF_VP8_STAGE_RECON) {
        hipLaunchKernelGGL(vp8_recon_kernel, dim3(hd.n_images), dim3(64 * BAND), 0, s, d_ims, scratch, recon, status);
        const int rl = maf_check_hip(hipGetLastError(), "vp8_recon launch");
        if (rl) return rl;
    }
    if (stages & MAF_VP8_STAGE_FILTER) {
        hipLaunchKernelGGL(vp8_filter_kernel, dim3(hd.n_images), dim3(64 * BAND), 0, s, d_ims, scratch, recon, yuv, status);
        const int rl = maf_check_hip(hipGetLastError(), "vp8_filter launch");
        if (rl) return rl;
    }
    if (stages & MAF_VP8_STAGE_CONVERT) {
        hipLaunchKernelGGL(vp8_convert_kernel, dim3((unsigned)((max_quads + 255) / 256), hd.n_images), dim3(256), 0, s, d_ims, yuv, out, status);
        const int rl = maf_check_hip(hipGetLastError(), "vp8_convert launch");
        if (rl) return rl;
    }
    return 0;
}
