// PNG decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to what cv2.imread (IMREAD_COLOR) asks libpng for,
// bit for bit (PNG is lossless: every conforming decoder gives the same samples; the conversion table is in maf-yolo_amd/png.py).  Replaces the
// cv2.imread of TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the png entries of IMG_FORMATS.
// The rules are restated in tests/png_ref.py; the host side (chunk walk, CRC-32, zlib header, blob) is maf-yolo_amd/png.py.
//
// Three kernels, one launch each for the whole batch (include/mafyolo_hip.h describes the blob and the buffers):
//   png_inflate_kernel    RFC 1951.  A deflate stream is one serial chain, so the batch is the parallelism: one one-wave workgroup per image.
//                         Symbol decoding is WAVE-UNIFORM: all 64 lanes hold the same bit window, compute the same table index and take the same
//                         branch, so the wave never diverges; the lanes differ only where bytes move.  Literals collect one per lane and are
//                         stored 64 at a time; a stored block is copied 64 bytes per step; a match of length L at distance D is
//                         out[p + i] = out[p - D + (i mod D)] for lanes i < L (also right for the overlapping case D < L), 64 bytes per step.
//                         Tables: the code-length code, the literal/length and the distance code of a dynamic block are built in LDS per block
//                         from canonical codes (counts and in-length ranks by wave ballots; a 9-bit first-level lookup filled entry-parallel,
//                         longer codes by a walk over first[l] / count[l], l = 10 .. 15); the fixed tables are built once per workgroup.
//                         WINDOW: the last 32 KiB of output live in an LDS ring (index = position mod 32768) and every byte is also stored to
//                         global memory as it is produced; a back-reference reads ONLY the ring, with a workgroup barrier between the lanes'
//                         ring writes and any later read (one wave per workgroup, so the barrier costs a wait on the LDS counter).  Global memory is
//                         never read back.
//   png_unfilter_kernel   Filter types 0 to 4.  One wave per image (per pass of an Adam7 image: each pass is a filter chain of its own, its first
//                         row with zeros above it) walks bands of 64 rows: lane k works on row y0 + k, one pixel behind lane
//                         k - 1, so the pixel above is what lane k - 1 produced one step ago (one shuffle) and the pixel above-left is the
//                         `above` of the lane's own previous step.  Lane 0 reads the row above the band from the output of the band before (workgroup fence + barrier
//                         between bands).  The next pixel's bytes are loaded one step ahead.
//   png_convert_kernel    One thread per 4 pixels: for an Adam7 image the gather (the pass from (x & 7, y & 7), the pixel's place in that pass's
//                         sub-image), strip 16 -> 8 (high byte), unpack 1 / 2 / 4 bit MSB first, gray x 255 / 85 / 17, palette from
//                         LDS, alpha dropped, BGR; 12 bytes out as three 32-bit stores.
//
// Bounded by construction (the inflate kernel reads bytes a file controls):
//   * input: every byte index is clamped into the stream section (which ends in zero padding) AND compared with the image's stream_end; past
//     it the reader feeds zeros, and consuming one of them sets MAF_PNG_ST_INPUT_EXHAUSTED and ends the stream;
//   * output: every store index is below inflated_size (the host-validated size of the image's region), every ring index is masked;
//   * a distance is compared with the bytes produced so far before anything is copied;
//   * loops: blocks <= 8 * stream bytes / 3 + 1 (a block header is 3 bits), symbols per block <= inflated_size + 1 (every symbol but the
//     end-of-block yields a byte), code lengths <= 320, stored bytes <= 65535, match bytes <= 258, rows <= h.  Nothing a file says is a
//     loop bound or an address without such a clamp.
// A malformed stream ends with status bits and a zero-filled remainder.
#include "maf_common.h"
#include "image_blob.h"

namespace {

constexpr int RING = 32768, RMASK = RING - 1;
constexpr int PNG_LOOK_BITS = 9, MAX_SYMS = 320;

__constant__ uint16_t k_len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
__constant__ uint8_t k_len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
__constant__ uint16_t k_dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                         8193, 12289, 16385, 24577};
__constant__ uint8_t k_dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
__constant__ uint8_t k_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// one canonical Huffman code in LDS
struct HuffTab {
    uint16_t look[1 << PNG_LOOK_BITS];   // (length << 9) | symbol for every 9-bit prefix (first stream bit = most significant) that starts with a code of at most 9 bits, else 0
    uint16_t sorted[MAX_SYMS];           // the symbols ordered by (length, symbol)
    int32_t first[16], count[16], offs[16];   // per length: the first code, the number of codes, the index of its first symbol in sorted[]
};

// The wave-uniform bit reader: every lane holds the same state.  Bits leave at the least significant end (RFC 1951 packing).
struct InflateBits {
    const uint8_t* buf;       // the stream section
    int64_t pos, end, last;   // next byte, one past the image's last byte, the last valid index of the section (inside the zero padding)
    uint64_t acc;             // the low n bits are unread
    int n;
    uint64_t word;            // the aligned 8 bytes of the section that hold byte 8 * widx ... (one load serves 8 byte reads)
    int64_t widx;

    __device__ __forceinline__ uint32_t byte_at(int64_t i) {
        i = i < 0 ? 0 : (i > last ? last : i);             // the clamp: whatever the stream says, the index stays inside the section
        const int64_t w = i >> 3;
        if (w != widx) {
            word = reinterpret_cast<const uint64_t*>(buf)[w];   // the section is 16-byte aligned and a multiple of 8 bytes long
            widx = w;
        }
        return (uint32_t)(word >> (8 * (int)(i & 7))) & 0xFFu;
    }
    __device__ __forceinline__ void fill() {               // at least 57 unread bits afterwards; pos moves on past `end` too, where zeros come in
        while (n <= 56) {
            const uint64_t b = pos < end ? byte_at(pos) : 0u;
            ++pos;
            acc |= b << n;
            n += 8;
        }
    }
    __device__ __forceinline__ int bits(int k) {           // k in [0, 16], n >= k
        const int v = (int)(acc & ((1u << k) - 1u));
        acc >>= k;
        n -= k;
        return v;
    }
    __device__ __forceinline__ bool exhausted() const { return (pos << 3) - n > (end << 3); }   // a bit past the image's stream has been consumed
};

// one symbol of code `t`; -1: no code matches.  Wave-uniform: the result goes through readfirstlane so that what follows branches on a scalar.
__device__ __forceinline__ int huff_symbol(InflateBits& br, const HuffTab& t) {
    br.fill();
    const uint32_t rev = __brev((uint32_t)br.acc & 0x7FFFu) >> 17;      // the next 15 bits, first stream bit most significant
    const uint32_t e = t.look[rev >> (15 - PNG_LOOK_BITS)];
    int sym = -1, len = 0;
    if (e) {
        len = (int)(e >> 9);
        sym = (int)(e & 511u);
    } else {
        for (int l = PNG_LOOK_BITS + 1; l <= 15; ++l) {
            const uint32_t d = (rev >> (15 - l)) - (uint32_t)t.first[l];
            if (d < (uint32_t)t.count[l]) {
                len = l;
                sym = t.sorted[t.offs[l] + (int)d];
                break;
            }
        }
    }
    len = __builtin_amdgcn_readfirstlane(len);
    br.acc >>= len;
    br.n -= len;
    return __builtin_amdgcn_readfirstlane(sym);
}

// Build `t` from the code lengths lens[0, nsym) (LDS, each 0 .. 15; nsym <= 320); called by the whole wave.  false: the code is over-subscribed, or
// incomplete where inflate does not allow it (zlib inftrees.c: an incomplete code passes only for a literal/length or distance code whose longest
// code has 1 bit).  Symbol j * 64 + lane is lane's j-th symbol, so a ballot per (j, length) gives counts and in-length ranks in symbol order.
__device__ bool build_table(HuffTab& t, const uint8_t* lens, int nsym, bool code_length_code, int lane) {
    int cnt[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int mylen[MAX_SYMS / 64], myrank[MAX_SYMS / 64];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < MAX_SYMS / 64; ++j) {
        const int s = j * 64 + lane;
        const int l = s < nsym ? (lens[s] & 15) : 0;
        mylen[j] = l;
        myrank[j] = 0;
#pragma unroll
        for (int b = 1; b < 16; ++b) {
            const uint64_t m = __ballot(l == b);
            if (l == b) myrank[j] = cnt[b] + __popcll(m & below);
            cnt[b] += __popcll(m);
        }
    }
    int left = 1, code = 0, off = 0, maxlen = 0, myfirst = 0, mycount = 0, myoffs = 0;
    bool over = false;
#pragma unroll
    for (int b = 1; b < 16; ++b) {
        code <<= 1;
        left = 2 * left - cnt[b];
        if (left < 0) { over = true; left = 0; }
        if (lane == b) { myfirst = code; mycount = cnt[b]; myoffs = off; }
        if (cnt[b]) maxlen = b;
        code += cnt[b];
        off += cnt[b];
    }
    if (lane < 16) { t.first[lane] = myfirst; t.count[lane] = mycount; t.offs[lane] = myoffs; }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < MAX_SYMS / 64; ++j)
        if (mylen[j]) t.sorted[min(t.offs[mylen[j]] + myrank[j], MAX_SYMS - 1)] = (uint16_t)(j * 64 + lane);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (1 << PNG_LOOK_BITS) / 64; ++k) {
        const int e = k * 64 + lane;
        uint32_t v = 0;
        for (int b = 1; b <= PNG_LOOK_BITS; ++b) {
            const uint32_t d = (uint32_t)(e >> (PNG_LOOK_BITS - b)) - (uint32_t)t.first[b];
            if (d < (uint32_t)t.count[b]) {
                v = ((uint32_t)b << 9) | t.sorted[min(t.offs[b] + (int)d, MAX_SYMS - 1)];
                break;
            }
        }
        t.look[e] = (uint16_t)v;
    }
    __syncthreads();
    return !over && (left == 0 || (!code_length_code && maxlen <= 1));
}

__global__ __launch_bounds__(64) void png_inflate_kernel(const maf_png_image_t* images, const uint8_t* streams, int64_t stream_bytes, uint8_t* inflated,
                                                          int32_t* status) {
    __shared__ uint8_t ring[RING];
    __shared__ HuffTab fixed_ll, fixed_d, dyn_ll, dyn_d, cl;
    __shared__ uint8_t lens[MAX_SYMS];
    const int lane = threadIdx.x;
    const maf_png_image_t im = images[blockIdx.x];
    const int total = im.inflated_size;
    uint8_t* out = inflated + im.inf_off;

    // the fixed code of RFC 1951 3.2.6, once per workgroup
    for (int s = lane; s < 288; s += 64) lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    __syncthreads();
    build_table(fixed_ll, lens, 288, false, lane);
    if (lane < 32) lens[lane] = 5;
    __syncthreads();
    build_table(fixed_d, lens, 32, false, lane);

    InflateBits br;
    br.buf = streams; br.pos = im.stream_begin; br.end = im.stream_end; br.last = stream_bytes - 1; br.acc = 0; br.n = 0; br.word = 0; br.widx = -1;
    int p = 0;                // bytes produced
    int st = 0;
    int nlit = 0;             // pending literals: lane k holds the k-th of them in `lit`
    uint32_t lit = 0;
    bool done = false;
    const int64_t max_blocks = (im.stream_end - im.stream_begin) * 8 / 3 + 1;

    // store the pending literals: ring and global memory, one byte per lane
    auto flush = [&]() {
        if (lane < nlit) {    // p + nlit <= total was checked when the literals were taken
            ring[(p + lane) & RMASK] = (uint8_t)lit;
            out[p + lane] = (uint8_t)lit;
        }
        p += nlit;
        nlit = 0;
        __syncthreads();      // the ring writes of all lanes come before any later read
    };

    for (int64_t blk = 0; blk < max_blocks && !st && !done; ++blk) {
        br.fill();
        const int bfinal = br.bits(1), btype = br.bits(2);
        if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
        if (btype == 3) { st |= MAF_PNG_ST_BAD_BLOCK_TYPE; break; }
        if (btype == 0) {
            br.bits(br.n & 7);                             // to the next byte boundary
            br.fill();
            const int len = br.bits(16);
            br.fill();
            const int nlen = br.bits(16);
            if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
            if ((len ^ 0xFFFF) != nlen) { st |= MAF_PNG_ST_BAD_STORED_LEN; break; }
            br.pos -= br.n >> 3;                           // hand the whole bytes still in the window back
            br.n = 0;
            br.acc = 0;
            const int take = min(len, total - p);
            for (int i = lane; i < take; i += 64) {        // take <= 65535
                const int64_t src = br.pos + i;
                const int64_t c = src < 0 ? 0 : (src > br.last ? br.last : src);
                const uint8_t b = src < br.end ? streams[c] : (uint8_t)0;
                ring[(p + i) & RMASK] = b;
                out[p + i] = b;
            }
            if (br.pos + len > br.end) st |= MAF_PNG_ST_INPUT_EXHAUSTED;
            if (len > take) st |= MAF_PNG_ST_TOO_MANY_BYTES;
            p += take;
            br.pos += len;
            __syncthreads();
            if (bfinal) done = true;
            continue;
        }
        const HuffTab* ll = &fixed_ll;
        const HuffTab* dd = &fixed_d;
        if (btype == 2) {
            br.fill();
            const int hlit = br.bits(5) + 257, hdist = br.bits(5) + 1, hclen = br.bits(4) + 4;
            if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
            if (hlit > 286 || hdist > 30) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }
            if (lane < 19) lens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < hclen; ++i) {              // hclen <= 19
                br.fill();
                const int v = br.bits(3);
                if (lane == 0) lens[k_cl_order[i]] = (uint8_t)v;
            }
            __syncthreads();
            if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
            if (!build_table(cl, lens, 19, true, lane)) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }
            const int nsym = hlit + hdist;                 // <= 316
            int n = 0, prev = 0;
            for (int it = 0; it < MAX_SYMS && n < nsym && !st; ++it) {   // every iteration adds at least one length
                const int s = huff_symbol(br, cl);
                int rep = 1, v = s;
                if (s < 0) { st |= MAF_PNG_ST_NO_CODE; break; }
                if (s == 16) {
                    if (n == 0) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }
                    rep = 3 + br.bits(2);
                    v = prev;
                } else if (s == 17) {
                    rep = 3 + br.bits(3);
                    v = 0;
                } else if (s == 18) {
                    rep = 11 + br.bits(7);
                    v = 0;
                }
                if (n + rep > nsym) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }
                for (int i = lane; i < rep; i += 64) lens[n + i] = (uint8_t)v;      // rep <= 138, n + rep <= 316
                n += rep;
                prev = v;
            }
            __syncthreads();
            if (br.exhausted()) st |= MAF_PNG_ST_INPUT_EXHAUSTED;
            if (st) break;
            if (lens[256] == 0) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }      // no end-of-block code
            const bool ok_ll = build_table(dyn_ll, lens, hlit, false, lane);
            const bool ok_d = build_table(dyn_d, lens + hlit, hdist, false, lane);
            if (!ok_ll || !ok_d) { st |= MAF_PNG_ST_BAD_CODE_LENGTHS; break; }
            ll = &dyn_ll;
            dd = &dyn_d;
        }
        bool eob = false;
        for (int it = 0; it <= total; ++it) {              // every iteration but the last yields at least one byte
            int s = huff_symbol(br, *ll);
            if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
            if (s < 0) { st |= MAF_PNG_ST_NO_CODE; break; }
            if (s < 256) {
                if (p + nlit >= total) { st |= MAF_PNG_ST_TOO_MANY_BYTES; break; }
                if (lane == nlit) lit = (uint32_t)s;
                if (++nlit == 64) flush();
                continue;
            }
            flush();
            if (s == 256) { eob = true; break; }
            if (s > 285) { st |= MAF_PNG_ST_NO_CODE; break; }
            s -= 257;
            const int L = k_len_base[s] + br.bits(k_len_extra[s]);
            const int ds = huff_symbol(br, *dd);
            if (ds < 0 || ds > 29) {
                st |= br.exhausted() ? MAF_PNG_ST_INPUT_EXHAUSTED : MAF_PNG_ST_NO_CODE;
                break;
            }
            const int D = k_dist_base[ds] + br.bits(k_dist_extra[ds]);
            if (br.exhausted()) { st |= MAF_PNG_ST_INPUT_EXHAUSTED; break; }
            if (D > p) { st |= MAF_PNG_ST_DISTANCE_TOO_FAR; break; }
            const int take = min(L, total - p);
            for (int i0 = 0; i0 < take; i0 += 64) {        // take <= 258
                const int i = i0 + lane;
                uint8_t b = 0;
                if (i < take) b = ring[(p - D + (D >= L ? i : i % D)) & RMASK];      // bytes before p only: all stored and behind a barrier
                __syncthreads();                           // every lane has read before any lane overwrites (D = 32768 shares the slot)
                if (i < take) {
                    ring[(p + i) & RMASK] = b;
                    out[p + i] = b;
                }
                __syncthreads();
            }
            p += take;
            if (L > take) { st |= MAF_PNG_ST_TOO_MANY_BYTES; break; }
        }
        flush();
        if (!eob && !st) st |= MAF_PNG_ST_TOO_MANY_BYTES;
        if (bfinal) done = true;
    }
    if (!done && !st) st |= MAF_PNG_ST_INPUT_EXHAUSTED;
    if (p < total) {
        if (!st) st |= MAF_PNG_ST_TOO_FEW_BYTES;
        for (int i = p + lane; i < total; i += 64) out[i] = 0;
    }
    if (st && lane == 0) atomicOr(&status[blockIdx.x], st);
}

__device__ __forceinline__ uint64_t load_px(const uint8_t* p, int bpp) {
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < bpp) v |= (uint64_t)p[j] << (8 * j);
    return v;
}

__device__ __forceinline__ uint64_t shfl_up1(uint64_t v) {
    const uint32_t lo = __shfl_up((uint32_t)v, 1), hi = __shfl_up((uint32_t)(v >> 32), 1);
    return ((uint64_t)hi << 32) | lo;
}

// Adam7 (PNG 1.2, 8.2): pass p holds the pixels (x0 + i * dx, y0 + j * dy) of the image as a sub-image of pw x ph pixels with rows of prb bytes,
// filtered on its own; the passes follow each other in the stream, and a pass without pixels is absent (no filter bytes either).
struct Adam7Pass {
    int x0, y0, dx, dy, pw, ph, prb;
};

__host__ __device__ inline Adam7Pass adam7_pass(int w, int h, int bits, int p) {
    constexpr int X0[7] = {0, 4, 0, 2, 0, 1, 0}, Y0[7] = {0, 0, 4, 0, 2, 0, 1}, DX[7] = {8, 8, 4, 4, 2, 2, 1}, DY[7] = {8, 8, 8, 4, 4, 2, 2};
    Adam7Pass g;
    g.x0 = X0[p]; g.y0 = Y0[p]; g.dx = DX[p]; g.dy = DY[p];
    g.pw = w > g.x0 ? (w - g.x0 + g.dx - 1) / g.dx : 0;
    g.ph = h > g.y0 ? (h - g.y0 + g.dy - 1) / g.dy : 0;
    g.prb = (int)(((int64_t)g.pw * bits + 7) / 8);
    return g;
}

// bytes of the passes in front of pass p: in the inflated stream (filter bytes included) and in the rows buffer (sub-images back to back)
__host__ __device__ inline void adam7_offsets(int w, int h, int bits, int p, int64_t& inf, int64_t& rows) {
    inf = rows = 0;
    for (int q = 0; q < p; ++q) {
        const Adam7Pass g = adam7_pass(w, h, bits, q);
        if (g.pw == 0 || g.ph == 0) continue;
        inf += (int64_t)g.ph * (1 + g.prb);
        rows += (int64_t)g.ph * g.prb;
    }
}

__host__ __device__ inline int png_channels(int ctype) { return ctype == 2 ? 3 : ctype == 4 ? 2 : ctype == 6 ? 4 : 1; }

// One filter chain: h rows of 1 + rb bytes at src -> h rows of rb bytes at dst, the row above the first is zeros.  Called by the whole wave with
// wave-uniform arguments (it holds workgroup barriers).  -> 1 in the lanes that met a filter type above 4.
__device__ __forceinline__ int unfilter_chain(const uint8_t* src, uint8_t* dst, int rb, int bpp, int h, int lane) {
    const int npx = rb / bpp;                                  // rowbytes is a multiple of bpp (bpp is 1 below 8 bits)
    int bad = 0;
    for (int y0 = 0; y0 < h; y0 += 64) {
        const int y = y0 + lane;
        const bool live = y < h;
        const uint8_t* in = src + (int64_t)min(y, h - 1) * (1 + rb);
        uint8_t* o = dst + (int64_t)min(y, h - 1) * rb;
        const uint8_t* above = dst + (int64_t)max(y0 - 1, 0) * rb;      // read by lane 0 of a band that is not the first
        int ft = live ? in[0] : 0;
        if (ft > 4) { bad = 1; ft = 0; }
        uint64_t left = 0, upleft = 0, prev_out = 0, pre = 0, up_pre = 0;
        for (int t = -1; t < npx + 63; ++t) {
            const int x = t - lane;
            const uint64_t raw = pre;
            uint64_t up = shfl_up1(prev_out);                  // what the lane of the row above produced one step ago: the same x
            if (lane == 0) up = up_pre;
            const bool nxt = live && x + 1 >= 0 && x + 1 < npx;
            pre = nxt ? load_px(in + 1 + (int64_t)(x + 1) * bpp, bpp) : 0;
            up_pre = (lane == 0 && y0 > 0 && nxt) ? load_px(above + (int64_t)(x + 1) * bpp, bpp) : 0;
            uint64_t cur = 0;
            if (live && x >= 0 && x < npx) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (j < bpp) {
                        const int a = (int)(left >> (8 * j)) & 255, b = (int)(up >> (8 * j)) & 255, c = (int)(upleft >> (8 * j)) & 255;
                        const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
                        const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                        const int pred = ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) >> 1 : ft == 4 ? paeth : 0;
                        const int v = ((int)(raw >> (8 * j)) + pred) & 255;
                        cur |= (uint64_t)v << (8 * j);
                        o[(int64_t)x * bpp + j] = (uint8_t)v;
                    }
                }
                upleft = up;
                left = cur;
            }
            prev_out = cur;
        }
        __threadfence_block();                                 // the band's last row is read by lane 0 in the next band
        __syncthreads();
    }
    return bad;
}

// grid (images, 1), or (images, 7) where the call holds an Adam7 file: workgroup (i, p) undoes pass p of image i, its own filter chain between
// its own offsets; for a plain image workgroup (i, 0) undoes the whole image and the others leave at once, as does that of an absent pass.
__global__ __launch_bounds__(64) void png_unfilter_kernel(const maf_png_image_t* images, const uint8_t* inflated, uint8_t* rows, int32_t* status) {
    const int lane = threadIdx.x;
    const maf_png_image_t im = images[blockIdx.x];
    const uint8_t* src = inflated + im.inf_off;
    uint8_t* dst = rows + im.rows_off;
    int bad;
    if (!im.interlace) {
        if (blockIdx.y) return;
        bad = unfilter_chain(src, dst, im.rowbytes, im.bpp, im.h, lane);
    } else {
        const int bits = png_channels(im.ctype) * im.depth;
        const Adam7Pass g = adam7_pass(im.w, im.h, bits, (int)blockIdx.y);
        if (g.pw == 0 || g.ph == 0) return;
        int64_t inf, sub;
        adam7_offsets(im.w, im.h, bits, (int)blockIdx.y, inf, sub);
        bad = unfilter_chain(src + inf, dst + sub, g.prb, im.bpp, g.ph, lane);
    }
    if (__any(bad) && lane == 0) atomicOr(&status[blockIdx.x], MAF_PNG_ST_BAD_FILTER);
}

__global__ __launch_bounds__(256) void png_convert_kernel(const maf_png_image_t* images, const uint32_t* palette, const uint8_t* rows, uint8_t* out,
                                                           int32_t* status) {
    __shared__ uint32_t lpal[256];
    __shared__ int64_t sub_off[7];                             // Adam7: where each pass's sub-image begins inside the image's rows, and its row length
    __shared__ int sub_rb[7];
    const maf_png_image_t im = images[blockIdx.y];
    const int tid = threadIdx.x;
    if ((int64_t)blockIdx.x * 1024 >= (int64_t)im.w * im.h) return;      // the grid is sized by the largest image of the call: a whole workgroup past this one leaves at once
    lpal[tid] = (im.ctype == 3 && tid < im.pal_n) ? palette[im.pal + tid] : 0u;
    const int w = im.w, depth = im.depth, ctype = im.ctype;
    const int chans = png_channels(ctype);
    const bool lace = im.interlace != 0;
    if (lace && tid < 7) {
        int64_t inf, sub;
        adam7_offsets(w, im.h, chans * depth, tid, inf, sub);
        sub_off[tid] = sub;
        sub_rb[tid] = adam7_pass(w, im.h, chans * depth, tid).prb;
    }
    __syncthreads();
    const int64_t npix = (int64_t)w * im.h;
    const int64_t q = ((int64_t)blockIdx.x * 256 + tid) * 4;
    if (q >= npix) return;
    const int n = (int)min((int64_t)4, npix - q);
    const int step = depth == 16 ? 2 : 1;                      // bytes per sample; byte 0 of a big-endian pair is the high byte
    const uint8_t* base = rows + im.rows_off;
    uint8_t px[12];
    int bad = 0;
    for (int j = 0; j < 4; ++j) {
        px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = 0;
        if (j >= n) continue;
        const int y = (int)((q + j) / w);
        int x = (int)((q + j) - (int64_t)y * w);
        const uint8_t* row = base + (int64_t)y * im.rowbytes;
        if (lace) {                                            // the gather: the pass from (x & 7, y & 7), then the pixel's place in that pass's sub-image
            const int p = (y & 1) ? 6 : (x & 1) ? 5 : (y & 2) ? 4 : (x & 2) ? 3 : (y & 4) ? 2 : (x & 4) ? 1 : 0;
            const Adam7Pass g = adam7_pass(w, im.h, 0, p);
            row = base + sub_off[p] + (int64_t)((y - g.y0) / g.dy) * sub_rb[p];
            x = (x - g.x0) / g.dx;
        }
        if (ctype == 2 || ctype == 6) {
            const uint8_t* s = row + (int64_t)x * chans * step;
            px[3 * j] = s[2 * step];
            px[3 * j + 1] = s[step];
            px[3 * j + 2] = s[0];
            continue;
        }
        int v;
        if (depth >= 8) {
            v = row[(int64_t)x * chans * step];
        } else {                                               // MSB first
            const int bit = x * depth;
            v = (row[bit >> 3] >> (8 - depth - (bit & 7))) & ((1 << depth) - 1);
        }
        if (ctype == 3) {
            uint32_t c = 0;
            if (v < im.pal_n) c = lpal[v]; else bad = 1;
            px[3 * j] = (uint8_t)c;
            px[3 * j + 1] = (uint8_t)(c >> 8);
            px[3 * j + 2] = (uint8_t)(c >> 16);
        } else {
            if (depth < 8) v *= 255 / ((1 << depth) - 1);      // x 255 / 85 / 17
            px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = (uint8_t)v;
        }
    }
    const int64_t o = im.out_off + 3 * q;                      // a multiple of 4: out_off is one of 16 and q one of 4
    if (n == 4) {
        uint32_t* d = reinterpret_cast<uint32_t*>(out + o);
        for (int k = 0; k < 3; ++k) d[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) out[o + k] = px[k];
    }
    if (bad) atomicOr(&status[blockIdx.y], MAF_PNG_ST_BAD_PALETTE_INDEX);
}

}  // namespace

extern "C" int maf_png_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "png_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_png_header_t); out[1] = (int32_t)sizeof(maf_png_image_t);
    return 0;
}

extern "C" int maf_png_decode(const void* blob_host, const void* blob_dev, uint8_t* inflated, uint8_t* rows, uint8_t* out, int32_t* status,
                              int32_t stages, maf_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && inflated && rows && out && status, "png_decode: null pointer");
    MAF_REQUIRE(stages > 0 && (stages & ~MAF_PNG_STAGE_ALL) == 0, "png_decode: stages is a mask of MAF_PNG_STAGE_*");
    MAF_REQUIRE(maf_aligned({blob_dev, inflated, rows, out}), "png_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_png_header_t hd = maf_blob_header<maf_png_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_images), "png_decode: 1 to 65535 images per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "png_decode: blob size out of range");
    MAF_REQUIRE(hd.n_palette >= 0 && hd.n_palette <= 256 * hd.n_images, "png_decode: palette entry count out of range");
    MAF_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_png_image_t), T) && in_blob(hd.palette_off, (int64_t)hd.n_palette * 4, T) &&
                in_blob(hd.stream_off, hd.stream_bytes, T) && hd.stream_bytes >= MAF_PNG_STREAM_PAD && hd.stream_bytes % 8 == 0,
                "png_decode: a blob section lies outside the blob");
    MAF_REQUIRE(hd.inflated_bytes > 0 && hd.rows_bytes > 0 && hd.out_bytes > 0, "png_decode: empty output buffers");
    const maf_png_image_t* ims = reinterpret_cast<const maf_png_image_t*>(hb + hd.images_off);
    const int64_t stream_data = hd.stream_bytes - MAF_PNG_STREAM_PAD;
    int64_t max_quads = 1;
    bool any_interlaced = false;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_png_image_t& m = ims[i];
        MAF_REQUIRE(m.w > 0 && m.h > 0 && m.w <= 65535 && m.h <= 65535, "png_decode: bad image size");
        const bool d8 = m.depth == 8 || m.depth == 16, dlow = m.depth == 1 || m.depth == 2 || m.depth == 4;
        MAF_REQUIRE((m.ctype == 0 && (d8 || dlow)) || (m.ctype == 3 && (m.depth == 8 || dlow)) || ((m.ctype == 2 || m.ctype == 4 || m.ctype == 6) && d8),
                    "png_decode: colour type and bit depth do not go together");
        const int chans = png_channels(m.ctype);
        const int64_t rowbits = (int64_t)m.w * chans * m.depth;
        MAF_REQUIRE(m.rowbytes == (rowbits + 7) / 8 && m.bpp == (chans * m.depth >= 8 ? chans * m.depth / 8 : 1), "png_decode: rowbytes or bpp does not match the image");
        MAF_REQUIRE(m.interlace == 0 || m.interlace == 1, "png_decode: interlace is 0 (none) or 1 (Adam7)");
        int64_t size = (int64_t)m.h * (1 + (int64_t)m.rowbytes), row_bytes = (int64_t)m.h * m.rowbytes;
        if (m.interlace) {
            adam7_offsets(m.w, m.h, chans * m.depth, 7, size, row_bytes);      // the sums over the non-empty passes
            any_interlaced = true;
        }
        MAF_REQUIRE(size < ((int64_t)1 << 31) && m.inflated_size == size, "png_decode: inflated size out of range");
        MAF_REQUIRE(m.stream_begin >= 0 && m.stream_begin <= m.stream_end && m.stream_end <= stream_data, "png_decode: an image's stream lies outside the stream section");
        MAF_REQUIRE(m.inf_off >= 0 && m.inf_off % 16 == 0 && m.inf_off <= hd.inflated_bytes && size <= hd.inflated_bytes - m.inf_off,
                    "png_decode: an image's scanlines lie outside the inflated buffer");
        MAF_REQUIRE(m.rows_off >= 0 && m.rows_off % 16 == 0 && m.rows_off <= hd.rows_bytes && row_bytes <= hd.rows_bytes - m.rows_off,
                    "png_decode: an image's rows lie outside the rows buffer");
        MAF_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off <= hd.out_bytes && (int64_t)3 * m.w * m.h <= hd.out_bytes - m.out_off,
                    "png_decode: a frame lies outside the output buffer");
        if (m.ctype == 3)
            MAF_REQUIRE(m.pal_n >= 1 && m.pal_n <= 256 && m.pal >= 0 && m.pal <= hd.n_palette - m.pal_n, "png_decode: an image's palette lies outside the palette section");
        const int64_t quads = ((int64_t)m.w * m.h + 3) / 4;
        max_quads = quads > max_quads ? quads : max_quads;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_png_image_t* d_ims = reinterpret_cast<const maf_png_image_t*>(db + hd.images_off);
    if (stages & MAF_PNG_STAGE_INFLATE) {
        const int rc = maf_check_hip(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s), "png_decode memset");
        if (rc) return rc;
        hipLaunchKernelGGL(png_inflate_kernel, dim3(hd.n_images), dim3(64), 0, s, d_ims, db + hd.stream_off, hd.stream_bytes, inflated, status);
        MAF_LAUNCH_CHECK("png_inflate");
    }
    if (stages & MAF_PNG_STAGE_UNFILTER) {
        hipLaunchKernelGGL(png_unfilter_kernel, dim3(hd.n_images, any_interlaced ? 7 : 1), dim3(64), 0, s, d_ims, inflated, rows, status);
        MAF_LAUNCH_CHECK("png_unfilter");
    }
    if (stages & MAF_PNG_STAGE_CONVERT) {
        hipLaunchKernelGGL(png_convert_kernel, dim3((unsigned)((max_quads + 255) / 256), hd.n_images), dim3(256), 0, s, d_ims,
                           reinterpret_cast<const uint32_t*>(db + hd.palette_off), rows, out, status);
        MAF_LAUNCH_CHECK("png_convert");
    }
    return 0;
}
