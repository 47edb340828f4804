// RFC 1951 inflate for one wave, shared by the codecs whose files carry deflate streams (png_decode.hip: the IDAT stream of an image;
// tiff_decode.hip: every Deflate strip, a zlib stream of its own).  Device code only; included inside the including file's anonymous namespace,
// behind maf_common.h.
//
// inflate_stream() is called by all 64 lanes of a one-wave workgroup with wave-uniform arguments (it holds workgroup barriers).  Symbol
// decoding is WAVE-UNIFORM: all 64 lanes hold the same bit window, compute the same table index and take the same branch, so the wave never
// diverges; the lanes differ only where bytes move.  Literals collect one per lane and are stored 64 at a time; a stored block is copied 64
// bytes per step; a match of length L at distance D is out[p + i] = out[p - D + (i mod D)] for lanes i < L (also right for the overlapping
// case D < L), 64 bytes per step.  Tables: the code-length code, the literal/length and the distance code of a dynamic block are built in
// LDS per block from canonical codes (counts and in-length ranks by wave ballots; a 9-bit first-level lookup filled entry-parallel, longer
// codes by a walk over first[l] / count[l], l = 10 .. 15); the fixed tables are built once per call.  WINDOW: the last 32 KiB of output live
// in an LDS ring (index = position mod 32768) and every byte is also stored to global memory as it is produced; a back-reference reads ONLY
// the ring, with a workgroup barrier between the lanes' ring writes and any later read.  Global memory is never read back.
//
// Bounded by construction (the stream is bytes a file controls):
//   * input: every byte index is clamped into the stream section (which ends in zero padding) AND compared with the stream's end; past it
//     the reader feeds zeros, and consuming one of them sets INFLATE_ST_INPUT_EXHAUSTED and ends the stream;
//   * output: every store index is below `total` (the host-validated size of the destination), every ring index is masked;
//   * a distance is compared with the bytes produced so far before anything is copied;
//   * loops: blocks <= 8 * stream bytes / 3 + 1 (a block header is 3 bits), symbols per block <= total + 1 (every symbol but the
//     end-of-block yields a byte), code lengths <= 320, stored bytes <= 65535, match bytes <= 258.
// A malformed stream ends with status bits and a zero-filled remainder.  The bits are those of MAF_PNG_ST_* (include/mafyolo_hip.h), which
// png_decode.hip hands on as they are.
#pragma once

enum : int {
    INFLATE_ST_INPUT_EXHAUSTED = 1, INFLATE_ST_BAD_BLOCK_TYPE = 2, INFLATE_ST_BAD_STORED_LEN = 4, INFLATE_ST_BAD_CODE_LENGTHS = 8, INFLATE_ST_NO_CODE = 16,
    INFLATE_ST_DISTANCE_TOO_FAR = 32, INFLATE_ST_TOO_MANY_BYTES = 64, INFLATE_ST_TOO_FEW_BYTES = 128
};

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

// everything inflate_stream keeps in LDS
struct InflateShared {
    uint8_t ring[RING];
    HuffTab fixed_ll, fixed_d, dyn_ll, dyn_d, cl;
    uint8_t lens[MAX_SYMS];
};

// Inflate the deflate stream streams[begin, end) (behind its zlib header; `streams` is a section of stream_bytes bytes, 16-byte aligned, a multiple
// of 8 long and zero-padded) into out[0, total) -> the INFLATE_ST_* bits (0: a whole stream of exactly `total` bytes).
__device__ __forceinline__ int inflate_stream(InflateShared& sh, const uint8_t* streams, int64_t stream_bytes, int64_t begin, int64_t end, uint8_t* out,
                                              int total, int lane) {
    // the fixed code of RFC 1951 3.2.6, once per workgroup
    for (int s = lane; s < 288; s += 64) sh.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : 8);
    __syncthreads();
    build_table(sh.fixed_ll, sh.lens, 288, false, lane);
    if (lane < 32) sh.lens[lane] = 5;
    __syncthreads();
    build_table(sh.fixed_d, sh.lens, 32, false, lane);

    InflateBits br;
    br.buf = streams; br.pos = begin; br.end = end; br.last = stream_bytes - 1; br.acc = 0; br.n = 0; br.word = 0; br.widx = -1;
    int p = 0;                // bytes produced
    int st = 0;
    int nlit = 0;             // pending literals: lane k holds the k-th of them in `lit`
    uint32_t lit = 0;
    bool done = false;
    const int64_t max_blocks = (end - begin) * 8 / 3 + 1;

    // store the pending literals: ring and global memory, one byte per lane
    auto flush = [&]() {
        if (lane < nlit) {    // p + nlit <= total was checked when the literals were taken
            sh.ring[(p + lane) & RMASK] = (uint8_t)lit;
            out[p + lane] = (uint8_t)lit;
        }
        p += nlit;
        nlit = 0;
        __syncthreads();      // the ring writes of all lanes come before any later read
    };

    for (int64_t blk = 0; blk < max_blocks && !st && !done; ++blk) {
        br.fill();
        const int bfinal = br.bits(1), btype = br.bits(2);
        if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
        if (btype == 3) { st |= INFLATE_ST_BAD_BLOCK_TYPE; break; }
        if (btype == 0) {
            br.bits(br.n & 7);                             // to the next byte boundary
            br.fill();
            const int len = br.bits(16);
            br.fill();
            const int nlen = br.bits(16);
            if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
            if ((len ^ 0xFFFF) != nlen) { st |= INFLATE_ST_BAD_STORED_LEN; break; }
            br.pos -= br.n >> 3;                           // hand the whole bytes still in the window back
            br.n = 0;
            br.acc = 0;
            const int take = min(len, total - p);
            for (int i = lane; i < take; i += 64) {        // take <= 65535
                const int64_t src = br.pos + i;
                const int64_t c = src < 0 ? 0 : (src > br.last ? br.last : src);
                const uint8_t b = src < br.end ? streams[c] : (uint8_t)0;
                sh.ring[(p + i) & RMASK] = b;
                out[p + i] = b;
            }
            if (br.pos + len > br.end) st |= INFLATE_ST_INPUT_EXHAUSTED;
            if (len > take) st |= INFLATE_ST_TOO_MANY_BYTES;
            p += take;
            br.pos += len;
            __syncthreads();
            if (bfinal) done = true;
            continue;
        }
        const HuffTab* ll = &sh.fixed_ll;
        const HuffTab* dd = &sh.fixed_d;
        if (btype == 2) {
            br.fill();
            const int hlit = br.bits(5) + 257, hdist = br.bits(5) + 1, hclen = br.bits(4) + 4;
            if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
            if (hlit > 286 || hdist > 30) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }
            if (lane < 19) sh.lens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < hclen; ++i) {              // hclen <= 19
                br.fill();
                const int v = br.bits(3);
                if (lane == 0) sh.lens[k_cl_order[i]] = (uint8_t)v;
            }
            __syncthreads();
            if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
            if (!build_table(sh.cl, sh.lens, 19, true, lane)) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }
            const int nsym = hlit + hdist;                 // <= 316
            int n = 0, prev = 0;
            for (int it = 0; it < MAX_SYMS && n < nsym && !st; ++it) {   // every iteration adds at least one length
                const int s = huff_symbol(br, sh.cl);
                int rep = 1, v = s;
                if (s < 0) { st |= INFLATE_ST_NO_CODE; break; }
                if (s == 16) {
                    if (n == 0) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }
                    rep = 3 + br.bits(2);
                    v = prev;
                } else if (s == 17) {
                    rep = 3 + br.bits(3);
                    v = 0;
                } else if (s == 18) {
                    rep = 11 + br.bits(7);
                    v = 0;
                }
                if (n + rep > nsym) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }
                for (int i = lane; i < rep; i += 64) sh.lens[n + i] = (uint8_t)v;      // rep <= 138, n + rep <= 316
                n += rep;
                prev = v;
            }
            __syncthreads();
            if (br.exhausted()) st |= INFLATE_ST_INPUT_EXHAUSTED;
            if (st) break;
            if (sh.lens[256] == 0) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }      // no end-of-block code
            const bool ok_ll = build_table(sh.dyn_ll, sh.lens, hlit, false, lane);
            const bool ok_d = build_table(sh.dyn_d, sh.lens + hlit, hdist, false, lane);
            if (!ok_ll || !ok_d) { st |= INFLATE_ST_BAD_CODE_LENGTHS; break; }
            ll = &sh.dyn_ll;
            dd = &sh.dyn_d;
        }
        bool eob = false;
        for (int it = 0; it <= total; ++it) {              // every iteration but the last yields at least one byte
            int s = huff_symbol(br, *ll);
            if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
            if (s < 0) { st |= INFLATE_ST_NO_CODE; break; }
            if (s < 256) {
                if (p + nlit >= total) { st |= INFLATE_ST_TOO_MANY_BYTES; break; }
                if (lane == nlit) lit = (uint32_t)s;
                if (++nlit == 64) flush();
                continue;
            }
            flush();
            if (s == 256) { eob = true; break; }
            if (s > 285) { st |= INFLATE_ST_NO_CODE; break; }
            s -= 257;
            const int L = k_len_base[s] + br.bits(k_len_extra[s]);
            const int ds = huff_symbol(br, *dd);
            if (ds < 0 || ds > 29) {
                st |= br.exhausted() ? INFLATE_ST_INPUT_EXHAUSTED : INFLATE_ST_NO_CODE;
                break;
            }
            const int D = k_dist_base[ds] + br.bits(k_dist_extra[ds]);
            if (br.exhausted()) { st |= INFLATE_ST_INPUT_EXHAUSTED; break; }
            if (D > p) { st |= INFLATE_ST_DISTANCE_TOO_FAR; break; }
            const int take = min(L, total - p);
            for (int i0 = 0; i0 < take; i0 += 64) {        // take <= 258
                const int i = i0 + lane;
                uint8_t b = 0;
                if (i < take) b = sh.ring[(p - D + (D >= L ? i : i % D)) & RMASK];      // bytes before p only: all stored and behind a barrier
                __syncthreads();                           // every lane has read before any lane overwrites (D = 32768 shares the slot)
                if (i < take) {
                    sh.ring[(p + i) & RMASK] = b;
                    out[p + i] = b;
                }
                __syncthreads();
            }
            p += take;
            if (L > take) { st |= INFLATE_ST_TOO_MANY_BYTES; break; }
        }
        flush();
        if (!eob && !st) st |= INFLATE_ST_TOO_MANY_BYTES;
        if (bfinal) done = true;
    }
    if (!done && !st) st |= INFLATE_ST_INPUT_EXHAUSTED;
    if (p < total) {
        if (!st) st |= INFLATE_ST_TOO_FEW_BYTES;
        for (int i = p + lane; i < total; i += 64) out[i] = 0;
    }
    return st;
}
