// Lossless WebP (VP8L) decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to libwebp's samples with alpha dropped,
// bit for bit (what cv2.imread (IMREAD_COLOR) asks libwebp for; the argument is in maf-yolo_amd/webp.py).  Replaces the cv2.imread of
// TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the webp entry of IMG_FORMATS, lossless files only.
// The rules are restated in tests/webp_ref.py; the host side (RIFF walk, the 5-byte header, blob) is maf-yolo_amd/webp.py; the blob, the buffers and
// the scratch layout are described in include/mafyolo_webp.h.
//
// Three kernels, one launch each for the whole batch:
//   webp_entropy_kernel    A VP8L stream is one serial chain, so the batch is the parallelism: one one-wave workgroup per image.  Control is
//                          WAVE-UNIFORM: all 64 lanes hold the same bit window, decode the same symbol and take the same branch; the lanes differ
//                          only where data moves (clearing and counting code lengths, placing a code's symbols by wave ballots, copies, cache
//                          updates).  It reads the transform headers, every sub-image, all prefix codes and the main image.
//                          CODES live in global memory (the arena of the image's scratch; the group count is known only once the entropy image is
//                          decoded): per code the count of every length and the symbols ordered by (length, symbol).  The five codes of the
//                          CURRENT group have their counts, and their symbols (at most 3136) in LDS; a symbol is found by the canonical walk over
//                          the lengths and one LDS load, so the pixel loop reads no table from global memory (group_symbol keeps the arena read for a
//                          record whose counts claim more symbols than an alphabet has).
//                          COPIES use all lanes: out[p + i] = out[p - D + (i mod D)] for lanes i < L, 64 pixels per step (right for D < L too: only
//                          pixels before p are read).  Unlike deflate's, a distance reaches ANY earlier pixel, so this kernel reads back global
//                          memory that the same wave wrote.  ORDER: a lane's load of a word comes behind another lane's earlier store of it
//                          because every path that stores pixels sets `dirty`, and a copy or a cache read first runs
//                          __threadfence_block() (the stores retired: a wait on the wave's outstanding memory operations plus a workgroup-scope
//                          release) and then __syncthreads() (one wave per workgroup, so the barrier is that wait) before its first load; the same
//                          pair stands between writing a code's record and the first symbol read from it, and at the end of every image.
//                          The last RING pixels also live in an LDS ring (index = position mod RING): a copy with D <= RING reads only the ring
//                          (a chunk's reads come before its writes, with a barrier between; chunk c reads positions >= p - RING + 64 c and the
//                          slots overwritten so far held positions below that), a longer one reads global memory.
//                          COLOUR CACHE in LDS.  Literals and cache hits are inserted by lane 0 (the value is wave-uniform); the pixels of a copy
//                          are inserted 64 at a time, and where two of them hash to one slot the LATER pixel must win: each lane raises the slot's
//                          tag to its position + 1 (atomicMax; positions only grow, so no tag is ever reset) and stores only if the tag is its own.
//   webp_transform_kernel  One wave per image, the transforms in the reverse of their reading order.  The predictor is the serial part: bands of
//                          64 rows, lane k on row y0 + k, TWO pixels behind lane k - 1, so the pixel above is what lane k - 1 produced two steps ago,
//                          the pixel above-right what it produced one step ago (two shuffles) and the pixel above-left the `above` of the lane's
//                          own previous step; at the last pixel of a row above-right is the row's own first pixel (the next word in memory).  Lane
//                          0 reads the row above the band from memory (fence + barrier between bands).  Four channels per step, in one 32-bit word.
//                          Cross-colour, add-green and index unpacking are element-wise.
//   webp_convert_kernel    One thread per 4 pixels: alpha dropped, BGR, 12 bytes out as three 32-bit stores; zeros for an image whose status is not 0.
//
// Bounded by construction (the entropy kernel reads bytes a file controls):
//   * input: every byte index is clamped into the stream section (which ends in zero padding) AND compared with the image's stream_end; past it
//     the reader feeds zeros, and once one of them is consumed every outcome is MAF_WEBP_ST_INPUT_EXHAUSTED;
//   * pixel stores: every index is below the pixel count of the image being read, which is w * h of the header the host validated, or a
//     sub-image's ceil(cw / 2^b) * ceil(h / 2^b) with b >= 2 and cw <= w (so at most S of the scratch layout), or the palette's n <= 256; ring,
//     cache and tag indices are masked;
//   * tables: a code's record and symbols are written only after arena_used + 18 + symbols <= arena_units and dir_used < dir_words were checked
//     (MAF_WEBP_ST_TABLE_SPACE otherwise); a symbol index inside a record is below the record's symbol count because both come from the same
//     code lengths, and is clamped all the same; the group index is at most the maximum the group count was taken from;
//   * loops: transforms <= 5 (the fifth repeats a type), groups <= 65536 and each costs 20 stream bits or fails on the zeros behind the stream,
//     code-length tokens <= alphabet <= 2328, a run is checked against the alphabet before it is written, cache bits 1 .. 11, palette <= 256,
//     a copy is checked against the pixels produced (distance) and the pixels left (length <= 4096) before anything moves, and every pass of the
//     pixel loop yields a pixel or ends the image.  Nothing a file says is a loop bound or an address without such a clamp.
// An image that ends with a non-zero status yields an all-zero frame.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include "image_blob.h"
#include "../../include/mafyolo_webp.h"

void maf_set_error(const std::string& msg);
int maf_check_hip(hipError_t e, const char* what);
#define WEBP_REQUIRE(cond, msg)              \
    do {                                     \
        if (!(cond)) {                       \
            maf_set_error(std::string(msg)); \
            return -1; /* MAF_E_ARG */       \
        }                                    \
    } while (0)

namespace {

constexpr int RING = 8192, RMASK = RING - 1;
constexpr int MAX_ALPHABET = 280 + 2048;
constexpr int REC = 18;                   // units of a code's record in front of its symbols
constexpr int KIND_NORMAL = 0, KIND_SINGLE = 1, KIND_FLAT = 2;
constexpr int META_WORDS = 64, PAL_WORDS = 256;
constexpr int SYM_LDS = 3200;              // symbols of the current group's codes kept in LDS: five full alphabets hold 2328 + 3 * 256 + 40 = 3136
constexpr uint32_t HASH_MUL = 0x1e35a7bdu;

__constant__ uint8_t k_cl_order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
__constant__ uint8_t k_plane[120] = {
    0x18, 0x07, 0x17, 0x19, 0x28, 0x06, 0x27, 0x29, 0x16, 0x1a, 0x26, 0x2a, 0x38, 0x05, 0x37, 0x39, 0x15, 0x1b, 0x36, 0x3a, 0x25, 0x2b, 0x48, 0x04,
    0x47, 0x49, 0x14, 0x1c, 0x35, 0x3b, 0x46, 0x4a, 0x24, 0x2c, 0x58, 0x45, 0x4b, 0x34, 0x3c, 0x03, 0x57, 0x59, 0x13, 0x1d, 0x56, 0x5a, 0x23, 0x2d,
    0x44, 0x4c, 0x55, 0x5b, 0x33, 0x3d, 0x68, 0x02, 0x67, 0x69, 0x12, 0x1e, 0x66, 0x6a, 0x22, 0x2e, 0x54, 0x5c, 0x43, 0x4d, 0x65, 0x6b, 0x32, 0x3e,
    0x78, 0x01, 0x77, 0x79, 0x53, 0x5d, 0x11, 0x1f, 0x64, 0x6c, 0x42, 0x4e, 0x76, 0x7a, 0x21, 0x2f, 0x75, 0x7b, 0x31, 0x3f, 0x63, 0x6d, 0x52, 0x5e,
    0x00, 0x74, 0x7c, 0x41, 0x4f, 0x10, 0x20, 0x62, 0x6e, 0x30, 0x73, 0x7d, 0x51, 0x5f, 0x40, 0x72, 0x7e, 0x61, 0x6f, 0x50, 0x71, 0x7f, 0x60, 0x70};

__host__ __device__ inline int subsample(int n, int b) { return (n + (1 << b) - 1) >> b; }

// the scratch layout of include/mafyolo_webp.h, in bytes
struct ScratchLayout {
    int64_t meta, palette, sub[3], pix[2], dir, arena, total;
};
__host__ __device__ inline ScratchLayout scratch_layout(int w, int h, int dir_words, int arena_units) {
    ScratchLayout s;
    const int64_t S = ((int64_t)subsample(w, 2) * subsample(h, 2) * 4 + 15) & ~(int64_t)15;
    s.meta = 0;
    s.palette = META_WORDS * 4;
    s.sub[0] = s.palette + PAL_WORDS * 4;
    s.sub[1] = s.sub[0] + S;
    s.sub[2] = s.sub[1] + S;
    const int64_t P = ((int64_t)w * h * 4 + 15) & ~(int64_t)15;
    s.pix[0] = s.sub[2] + S;
    s.pix[1] = s.pix[0] + P;
    s.dir = s.pix[1] + P;
    s.arena = s.dir + (((int64_t)dir_words * 4 + 15) & ~(int64_t)15);
    s.total = s.arena + (((int64_t)arena_units * 2 + 15) & ~(int64_t)15);
    return s;
}

// The wave-uniform bit reader: every lane holds the same state.  Bits leave at the least significant end.
struct WebpBits {
    const uint8_t* buf;       // the stream section
    int64_t pos, end, last;   // next byte, one past the image's last byte, the last valid index of the section (inside the zero padding)
    uint64_t acc;             // the low n bits are unread
    int n;
    uint64_t word;            // the aligned 8 bytes of the section that hold byte 8 * widx ...
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
    __device__ __forceinline__ int bits(int k) {           // k in [0, 24]
        fill();
        const int v = (int)(acc & ((1ull << k) - 1ull));
        acc >>= k;
        n -= k;
        return v;
    }
    __device__ __forceinline__ bool exhausted() const { return (pos << 3) - n > (end << 3); }   // a bit past the image's stream has been consumed
};

// the five codes of the current group: the record heads, in LDS
struct GroupLds {
    uint16_t cnt[5][16];
    int32_t off[5], kind[5], single[5];
    int32_t lds_at[5];        // where the code's symbols begin in Shared::syms; -1: none there (no stored symbols, or a record that claims more than fit)
};

struct Shared {
    uint32_t ring[RING];
    uint32_t cache[2048];
    uint32_t tag[2048];
    uint8_t lens[MAX_ALPHABET + 8];
    uint16_t syms[SYM_LDS];
    int32_t count[16];
    uint16_t cl_cnt[16], cl_sorted[20];
    uint8_t cl_len[20];
    int32_t found;
    GroupLds g;
};

// what the whole wave knows about the image it decodes
struct Decoder {
    WebpBits br;
    Shared* sh;
    uint32_t* dir;
    uint16_t* arena;
    int dir_words, arena_units, dir_used, arena_used;
    int st, lane;

    __device__ __forceinline__ void fail(int bit) {
        if (!st) st = br.exhausted() ? MAF_WEBP_ST_INPUT_EXHAUSTED : bit;
    }
    __device__ __forceinline__ void order() {              // stores retired, then the barrier (the header comment's ORDER)
        __threadfence_block();
        __syncthreads();
    }
};

// One symbol by the canonical walk: cnt[l] codes of length l, the symbols of a length in order behind those of the shorter ones.  -> the
// symbol's index among the used symbols, -1: no code matches.  Wave-uniform.
__device__ __forceinline__ int walk_code(WebpBits& br, const uint16_t* cnt) {
    br.fill();
    const uint32_t window = (uint32_t)br.acc;
    int code = 0, first = 0, index = 0, len = 0, found = -1;
    for (int l = 1; l <= 15; ++l) {
        code |= (int)((window >> (l - 1)) & 1u);
        const int c = cnt[l];
        if (code - first < c) {
            found = index + code - first;
            len = l;
            break;
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    len = __builtin_amdgcn_readfirstlane(len);
    br.acc >>= len;
    br.n -= len;
    return __builtin_amdgcn_readfirstlane(found);
}

// one symbol of code k of the current group
__device__ __forceinline__ int group_symbol(Decoder& d, int k) {
    const GroupLds& g = d.sh->g;
    if (g.kind[k] == KIND_SINGLE) return g.single[k];      // a one-symbol code consumes no bits
    const int idx = walk_code(d.br, g.cnt[k]);
    if (idx < 0) {
        d.fail(MAF_WEBP_ST_NO_CODE);
        return 0;
    }
    if (g.kind[k] == KIND_FLAT) return idx;
    if (g.lds_at[k] >= 0) return __builtin_amdgcn_readfirstlane((int)d.sh->syms[min(g.lds_at[k] + idx, SYM_LDS - 1)]);
    const int64_t at = (int64_t)g.off[k] + REC + idx;
    return __builtin_amdgcn_readfirstlane((int)d.arena[at < d.arena_units ? at : d.arena_units - 1]);
}

// bring the record heads of the five codes dir[base .. base + 5) into LDS, and their symbols as far as SYM_LDS holds them
__device__ __forceinline__ void load_group(Decoder& d, int base) {
    GroupLds& g = d.sh->g;
    __syncthreads();
    for (int k = d.lane; k < 80; k += 64) {
        const int c = k >> 4, j = k & 15;
        const int e = min(base + c, d.dir_used - 1);
        const int64_t o = min((int64_t)d.dir[e], (int64_t)d.arena_units - REC);
        const uint16_t v = d.arena[o + j];
        if (j == 0) {
            g.off[c] = (int)o;
            g.kind[c] = v;
            g.single[c] = d.arena[o + 16];
            g.cnt[c][0] = 0;
        } else {
            g.cnt[c][j] = v;
        }
    }
    __syncthreads();
    // every lane: where each code's symbols go (n comes from the record: whatever it says, the copy stays inside syms)
    int at[5], n[5], total = 0;
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        int m = 0;
        if (g.kind[c] == KIND_NORMAL)
            for (int l = 1; l <= 15; ++l) m += g.cnt[c][l];
        const bool fits = m > 0 && m <= SYM_LDS - total;
        n[c] = fits ? m : 0;
        at[c] = fits ? total : -1;
        total += n[c];
    }
    for (int i = d.lane; i < total; i += 64) {                 // one pass over the symbols of all five codes: total <= SYM_LDS
        int c = 0, first = at[0];
#pragma unroll
        for (int k = 1; k < 5; ++k)
            if (at[k] >= 0 && i >= at[k]) {
                c = k;
                first = at[k];
            }
        const int64_t from = (int64_t)g.off[c] + REC + (i - first);
        d.sh->syms[i] = d.arena[min(from, (int64_t)d.arena_units - 1)];
    }
    if (d.lane < 5) {
        int v = at[0];
#pragma unroll
        for (int k = 1; k < 5; ++k)
            if (d.lane == k) v = at[k];
        g.lds_at[d.lane] = v;
    }
    __syncthreads();
}

// Read one prefix code over `alphabet` symbols, write its record into the arena and its place into dir[dir_used++].
__device__ __forceinline__ void read_code(Decoder& d, int alphabet) {
    Shared& sh = *d.sh;
    WebpBits& br = d.br;
    const int lane = d.lane;
    if (d.st) return;
    if (d.dir_used >= d.dir_words) { d.fail(MAF_WEBP_ST_TABLE_SPACE); return; }
    for (int s = lane; s < alphabet; s += 64) sh.lens[s] = 0;
    if (lane < 16) sh.count[lane] = 0;
    if (lane == 0) sh.found = 0;
    __syncthreads();
    bool flat = false;
    if (br.bits(1)) {                                          // simple
        const int k = br.bits(1) + 1;
        const int first8 = br.bits(1);
        const int s0 = br.bits(first8 ? 8 : 1);
        const int s1 = k == 2 ? br.bits(8) : s0;
        if (s0 >= alphabet || s1 >= alphabet) { d.fail(MAF_WEBP_ST_BAD_CODE_LENGTHS); return; }
        if (lane == 0) {
            sh.lens[s0] = 1;
            sh.lens[s1] = 1;
        }
    } else {
        const int ncl = 4 + br.bits(4);                        // <= 19
        if (lane < 20) sh.cl_len[lane] = 0;
        if (lane < 16) sh.cl_cnt[lane] = 0;
        __syncthreads();
        for (int i = 0; i < ncl; ++i) {
            const int v = br.bits(3);
            if (lane == 0) sh.cl_len[k_cl_order[i]] = (uint8_t)v;
        }
        __syncthreads();
        if (lane == 0) {                                       // the code-length code: 19 symbols, built by one lane
            int n = 0;
            for (int l = 1; l <= 7; ++l) {
                int c = 0;
                for (int s = 0; s < 19; ++s)
                    if (sh.cl_len[s] == l) {
                        sh.cl_sorted[n++] = (uint16_t)s;       // n <= 19
                        ++c;
                    }
                sh.cl_cnt[l] = (uint16_t)c;
            }
        }
        __syncthreads();
        int used = 0, left = 1;
        bool over = false;
        for (int l = 1; l <= 15; ++l) {
            used += sh.cl_cnt[l];
            left = 2 * left - sh.cl_cnt[l];
            if (left < 0) { over = true; left = 0; }
        }
        const int cl_single = used == 1 ? (int)sh.cl_sorted[0] : -1;
        if (cl_single < 0 && (over || left != 0 || used == 0)) { d.fail(MAF_WEBP_ST_BAD_CODE_LENGTHS); return; }
        flat = cl_single >= 1 && cl_single <= 15;
        int max_symbol = alphabet;
        if (br.bits(1)) {
            const int nb = 2 + 2 * br.bits(3);                 // <= 16
            max_symbol = 2 + br.bits(nb);
            if (max_symbol > alphabet) { d.fail(MAF_WEBP_ST_BAD_CODE_LENGTHS); return; }
        }
        int s = 0, prev = 8;
        for (int it = 0; it < alphabet && s < alphabet && max_symbol > 0 && !d.st; ++it) {   // every token adds at least one length
            --max_symbol;
            int t = cl_single;
            if (t < 0) {
                const int idx = walk_code(br, sh.cl_cnt);
                if (idx < 0) { d.fail(MAF_WEBP_ST_NO_CODE); break; }
                t = sh.cl_sorted[min(idx, 18)];
            }
            int rep = 1, v = t;
            if (t == 16) {
                rep = 3 + br.bits(2);
                v = prev;
            } else if (t == 17) {
                rep = 3 + br.bits(3);
                v = 0;
            } else if (t == 18) {
                rep = 11 + br.bits(7);
                v = 0;
            } else if (t) {
                prev = t;
            }
            if (s + rep > alphabet) { d.fail(MAF_WEBP_ST_BAD_CODE_LENGTHS); break; }
            for (int i = lane; i < rep; i += 64) sh.lens[s + i] = (uint8_t)v;     // rep <= 138, s + rep <= alphabet
            s += rep;
        }
        if (d.st) return;
    }
    __syncthreads();
    // counts per length, the one symbol of a one-symbol code
    for (int s = lane; s < alphabet; s += 64) {
        const int l = sh.lens[s] & 15;
        if (l) {
            atomicAdd(&sh.count[l], 1);
            sh.found = s;                                      // any used symbol: meant for the code that has one
        }
    }
    __syncthreads();
    int cnt[16], offs[16];
    int used = 0, left = 1;
    bool over = false;
#pragma unroll
    for (int l = 1; l <= 15; ++l) {
        cnt[l] = sh.count[l];
        offs[l] = used;
        used += cnt[l];
        left = 2 * left - cnt[l];
        if (left < 0) { over = true; left = 0; }
    }
    cnt[0] = offs[0] = 0;
    if (used != 1 && (over || left != 0 || used == 0)) { d.fail(MAF_WEBP_ST_BAD_CODE_LENGTHS); return; }
    if (br.exhausted()) { d.fail(MAF_WEBP_ST_INPUT_EXHAUSTED); return; }
    const int kind = used == 1 ? KIND_SINGLE : flat ? KIND_FLAT : KIND_NORMAL;
    const int need = REC + (kind == KIND_NORMAL ? used : 0);
    if (need > d.arena_units - d.arena_used) { d.fail(MAF_WEBP_ST_TABLE_SPACE); return; }
    const int base = d.arena_used;
    uint16_t* rec = d.arena + base;
    if (lane < REC) rec[lane] = (uint16_t)(lane == 0 ? kind : lane < 16 ? sh.count[lane] : lane == 16 ? sh.found : 0);
    if (kind == KIND_NORMAL) {
        // symbol j * 64 + lane is lane's j-th symbol, so a ballot per (j, length) gives the in-length ranks in symbol order
        const uint64_t below = (1ull << lane) - 1ull;
        int run[16];
#pragma unroll
        for (int l = 0; l < 16; ++l) run[l] = 0;
        for (int s0 = 0; s0 < alphabet; s0 += 64) {
            const int s = s0 + lane;
            const int l = s < alphabet ? (sh.lens[s] & 15) : 0;
#pragma unroll
            for (int b = 1; b <= 15; ++b) {
                const uint64_t m = __ballot(l == b);
                if (l == b) rec[REC + min(offs[b] + run[b] + (int)__popcll(m & below), used - 1)] = (uint16_t)s;
                run[b] += __popcll(m);
            }
        }
    }
    if (lane == 0) d.dir[d.dir_used] = (uint32_t)base;
    d.dir_used += 1;
    d.arena_used += need;
    d.order();                                                 // the record is read back by every lane
}

__device__ __forceinline__ int prefix_value(WebpBits& br, int p) {      // p < 40: the extra bits are at most 18
    if (p < 4) return p + 1;
    const int e = (p - 2) >> 1;
    return ((2 + (p & 1)) << e) + br.bits(e) + 1;
}

// One entropy-coded image of w x h pixels -> dst[0, w * h).  MAIN: the main image (it may have meta codes: an entropy image in `meta_dst`).
template <bool MAIN>
__device__ __forceinline__ void read_image(Decoder& d, int w, int h, uint32_t* dst, uint32_t* meta_dst) {
    Shared& sh = *d.sh;
    WebpBits& br = d.br;
    const int lane = d.lane;
    if (d.st) return;
    int cache_bits = 0;
    if (br.bits(1)) {
        cache_bits = br.bits(4);
        if (cache_bits < 1 || cache_bits > 11) { d.fail(MAF_WEBP_ST_BAD_CACHE_BITS); return; }
    }
    const int csize = cache_bits ? 1 << cache_bits : 0;
    int groups = 1, pb = 0, mw = 0;
    bool meta = false;
    if (MAIN) {
        if (br.bits(1)) {
            meta = true;
            pb = br.bits(3) + 2;
            mw = subsample(w, pb);
            const int mh = subsample(h, pb);
            read_image<false>(d, mw, mh, meta_dst, nullptr);
            if (d.st) return;
            int mx = 0;
            for (int i = lane; i < mw * mh; i += 64) mx = max(mx, (int)((meta_dst[i] >> 8) & 0xFFFFu));
            for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
            groups = __builtin_amdgcn_readfirstlane(mx) + 1;   // <= 65536
        }
    }
    const int set_base = d.dir_used;
    for (int g = 0; g < groups && !d.st; ++g) {
        for (int k = 0; k < 5; ++k) read_code(d, k == 0 ? 280 + csize : k == 4 ? 40 : 256);      // green / length / cache, red, blue, alpha, distance
    }
    if (d.st) return;
    for (int i = lane; i < 2048; i += 64) {
        sh.cache[i] = 0;
        sh.tag[i] = 0;
    }
    const int n = w * h;
    int p = 0, x = 0, y = 0, cur_group = -1, cur_block = -1;
    bool dirty = true;
    while (p < n && !d.st) {                                   // every pass yields at least one pixel or sets st
        int gi = 0;
        if (meta) {
            const int blk = (y >> pb) * mw + (x >> pb);        // inside the entropy image: x < w, y < h
            if (blk != cur_block) {
                cur_block = blk;
                gi = (int)((meta_dst[blk] >> 8) & 0xFFFFu);
                gi = __builtin_amdgcn_readfirstlane(min(gi, groups - 1));
            } else {
                gi = cur_group;
            }
        }
        if (gi != cur_group) {
            load_group(d, set_base + 5 * gi);
            cur_group = gi;
        }
        const int s = group_symbol(d, 0);
        if (d.st) break;
        int produced = 1;
        if (s < 256 || s >= 280) {
            uint32_t argb;
            if (s < 256) {
                const int r = group_symbol(d, 1);
                const int b = group_symbol(d, 2);
                const int a = group_symbol(d, 3);
                if (d.st) break;
                argb = ((uint32_t)a << 24) | ((uint32_t)(r & 255) << 16) | ((uint32_t)s << 8) | (uint32_t)(b & 255);
            } else {
                if (dirty) { d.order(); dirty = false; }
                argb = sh.cache[(s - 280) & (csize - 1) & 2047];          // s - 280 < csize by the alphabet; csize >= 2 here
                __syncthreads();                                          // every lane has read before lane 0 writes below
            }
            if (br.exhausted()) { d.fail(MAF_WEBP_ST_INPUT_EXHAUSTED); break; }
            if (lane == 0) {
                dst[p] = argb;
                sh.ring[p & RMASK] = argb;
                if (csize) sh.cache[((HASH_MUL * argb) >> (32 - cache_bits)) & 2047] = argb;
            }
            dirty = true;
        } else {
            const int L = prefix_value(br, s - 256);                      // <= 4096
            const int ds = group_symbol(d, 4);
            if (d.st) break;
            const int dc = prefix_value(br, min(ds, 39));                 // <= 2^20
            int D;
            if (dc > 120) {
                D = dc - 120;
            } else {
                const int k = k_plane[dc - 1];
                D = (k >> 4) * w + 8 - (k & 15);
                if (D < 1) D = 1;
            }
            if (br.exhausted()) { d.fail(MAF_WEBP_ST_INPUT_EXHAUSTED); break; }
            if (D > p) { d.fail(MAF_WEBP_ST_DISTANCE_TOO_FAR); break; }
            if (L > n - p) { d.fail(MAF_WEBP_ST_COPY_PAST_END); break; }
            if (dirty) { d.order(); dirty = false; }
            const bool near = D <= RING;
            for (int i0 = 0; i0 < L; i0 += 64) {                          // L <= 4096
                const int i = i0 + lane;
                uint32_t v = 0;
                if (i < L) {
                    const int src = p - D + (D >= L ? i : i % D);         // pixels before p only: all stored and behind the order() above
                    v = near ? sh.ring[src & RMASK] : dst[src];
                }
                __syncthreads();                                          // every lane has read before any lane overwrites a ring slot
                const uint32_t key = ((HASH_MUL * v) >> (32 - (cache_bits ? cache_bits : 1))) & 2047;
                if (i < L) {
                    sh.ring[(p + i) & RMASK] = v;
                    dst[p + i] = v;                                       // p + i < p + L <= n
                    if (csize) atomicMax(&sh.tag[key], (uint32_t)(p + i + 1));
                }
                __syncthreads();
                if (csize && i < L && sh.tag[key] == (uint32_t)(p + i + 1)) sh.cache[key] = v;      // the later pixel of a slot wins
                __syncthreads();
            }
            produced = L;
            dirty = true;
        }
        p += produced;
        x += produced;
        while (x >= w) {                                       // produced <= 4096
            x -= w;
            ++y;
        }
        if (br.exhausted()) d.fail(MAF_WEBP_ST_INPUT_EXHAUSTED);
    }
    d.order();
}

// the transform record in the scratch's first words: [0] transforms, [1] coded width, [2] which buffer holds the final image (0 argb, 1 / 2 the
// scratch's), then per transform in reading order 8 words: type, bits, width it works on, byte offset of its data in the scratch, palette size
constexpr int TR_AT = 8, TR_STRIDE = 8;

__global__ __launch_bounds__(64) void webp_entropy_kernel(const maf_webp_image_t* images, const uint8_t* streams, int64_t stream_bytes, uint32_t* argb,
                                                           uint8_t* scratch, int32_t* status) {
    __shared__ Shared sh;
    const maf_webp_image_t im = images[blockIdx.x];
    uint8_t* sc = scratch + im.scratch_off;
    const ScratchLayout lay = scratch_layout(im.w, im.h, im.dir_words, im.arena_units);
    uint32_t* rec = reinterpret_cast<uint32_t*>(sc + lay.meta);
    uint32_t* palette = reinterpret_cast<uint32_t*>(sc + lay.palette);
    Decoder d;
    d.br.buf = streams; d.br.pos = im.stream_begin; d.br.end = im.stream_end; d.br.last = stream_bytes - 1;
    d.br.acc = 0; d.br.n = 0; d.br.word = 0; d.br.widx = -1;
    d.sh = &sh;
    d.dir = reinterpret_cast<uint32_t*>(sc + lay.dir);
    d.arena = reinterpret_cast<uint16_t*>(sc + lay.arena);
    d.dir_words = im.dir_words; d.arena_units = im.arena_units; d.dir_used = 0; d.arena_used = 0;
    d.st = 0; d.lane = threadIdx.x;
    const int lane = d.lane;
    const int w = im.w, h = im.h;
    int cw = w, ntr = 0, seen = 0;
    for (int it = 0; it < 5 && !d.st; ++it) {                  // four types, each at most once: a fifth header repeats one
        if (!d.br.bits(1)) break;
        const int t = d.br.bits(2);
        if (seen & (1 << t)) { d.fail(MAF_WEBP_ST_BAD_TRANSFORM); break; }
        seen |= 1 << t;
        int b = 0, pal_n = 0;
        int64_t data = 0;
        const int tw = cw;
        if (t < 2) {
            b = d.br.bits(3) + 2;
            data = lay.sub[t];
            read_image<false>(d, subsample(cw, b), subsample(h, b), reinterpret_cast<uint32_t*>(sc + data), nullptr);   // <= S pixels
        } else if (t == 3) {
            pal_n = d.br.bits(8) + 1;                          // <= 256
            data = lay.palette;
            read_image<false>(d, pal_n, 1, palette, nullptr);
            if (!d.st && lane == 0) {                          // per-channel cumulative addition
                uint32_t acc = 0;
                for (int i = 0; i < pal_n; ++i) {
                    const uint32_t v = palette[i];
                    acc = (((acc & 0xFF00FF00u) + (v & 0xFF00FF00u)) & 0xFF00FF00u) | (((acc & 0x00FF00FFu) + (v & 0x00FF00FFu)) & 0x00FF00FFu);
                    palette[i] = acc;
                }
            }
            b = pal_n <= 2 ? 3 : pal_n <= 4 ? 2 : pal_n <= 16 ? 1 : 0;
            cw = subsample(cw, b);
        }
        if (d.st) break;
        if (lane == 0) {
            uint32_t* r = rec + TR_AT + TR_STRIDE * ntr;       // ntr <= 3
            r[0] = (uint32_t)t; r[1] = (uint32_t)b; r[2] = (uint32_t)tw; r[3] = (uint32_t)data; r[4] = (uint32_t)pal_n;
        }
        ++ntr;
        if (d.br.exhausted()) d.fail(MAF_WEBP_ST_INPUT_EXHAUSTED);
    }
    read_image<true>(d, cw, h, argb + im.argb_off, reinterpret_cast<uint32_t*>(sc + lay.sub[2]));
    if (!d.st && d.br.exhausted()) d.st = MAF_WEBP_ST_INPUT_EXHAUSTED;
    if (lane == 0) {
        rec[0] = (uint32_t)ntr; rec[1] = (uint32_t)cw; rec[2] = 0;
        if (d.st) atomicOr(&status[blockIdx.x], d.st);
    }
}

// ---------------------------------------------------------------- inverse transforms

__device__ __forceinline__ uint32_t avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xFEFEFEFEu) >> 1) + (a & b); }
__device__ __forceinline__ uint32_t add_px(uint32_t a, uint32_t b) {
    return (((a & 0xFF00FF00u) + (b & 0xFF00FF00u)) & 0xFF00FF00u) | (((a & 0x00FF00FFu) + (b & 0x00FF00FFu)) & 0x00FF00FFu);
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
        default: return 0xFF000000u;                           // 0, and 14 / 15 as libwebp's guard entries
    }
}

// residuals in `in`, pixels out to px (w x h; px == in works in place); blocks: the sub-image of modes.  Called by the whole wave.
__device__ void inverse_predictor(const uint32_t* in, uint32_t* px, int w, int h, int b, const uint32_t* blocks, int lane) {
    const int bw = subsample(w, b), bmask = (1 << b) - 1;
    for (int y0 = 0; y0 < h; y0 += 64) {
        const int y = y0 + lane;
        const bool live = y < h;
        uint32_t* row = px + (int64_t)min(y, h - 1) * w;
        const uint32_t* rin = in + (int64_t)min(y, h - 1) * w;
        const uint32_t* above = px + (int64_t)max(y0 - 1, 0) * w;        // read by lane 0 of a band that is not the first
        uint32_t left = 0, tl = 0, o1 = 0, o2 = 0, first = 0, pre = 0;
        int mode = 0;
        if (live) pre = rin[0];
        for (int t = 0; t < w + 126; ++t) {
            const int x = t - 2 * lane;
            uint32_t T = __shfl_up(o2, 1), TR = __shfl_up(o1, 1);        // lane k - 1 two steps / one step ago: the same x, x + 1
            const bool on = live && x >= 0 && x < w;
            const uint32_t res = pre;
            if (live && x + 1 >= 0 && x + 1 < w) pre = rin[x + 1];
            uint32_t cur = 0;
            if (on) {
                if (lane == 0 && y0 > 0) {
                    T = above[x];
                    TR = x + 1 < w ? above[x + 1] : 0;
                }
                if (x == w - 1) TR = first;                    // the next word in memory: this row's first pixel
                uint32_t pred;
                if (y == 0) {
                    pred = x == 0 ? 0xFF000000u : left;
                } else if (x == 0) {
                    pred = T;
                } else {
                    if (x == 1 || (x & bmask) == 0) mode = (int)(blocks[(y >> b) * bw + (x >> b)] >> 8) & 15;
                    pred = predict(mode, left, T, tl, TR);
                }
                cur = add_px(res, pred);
                row[x] = cur;
                if (x == 0) first = cur;
                left = cur;
                tl = T;
            }
            o2 = o1;
            o1 = cur;
        }
        __threadfence_block();                                 // the band's last row is read by lane 0 in the next band
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void webp_transform_kernel(const maf_webp_image_t* images, uint32_t* argb, uint8_t* scratch, const int32_t* status) {
    const maf_webp_image_t im = images[blockIdx.x];
    if (status[blockIdx.x]) return;
    const int lane = threadIdx.x;
    uint8_t* sc = scratch + im.scratch_off;
    const ScratchLayout lay = scratch_layout(im.w, im.h, im.dir_words, im.arena_units);
    uint32_t* rec = reinterpret_cast<uint32_t*>(sc + lay.meta);
    const int ntr = min((int)rec[0], 4), h = im.h;
    // argb keeps the entropy stage's pixels (the tap): the first transform writes into a buffer of the scratch, the later ones work in place
    // there, and colour indexing, which widens rows, always moves to the other buffer
    const uint32_t* cur = argb + im.argb_off;
    uint32_t* bufs[2] = {reinterpret_cast<uint32_t*>(sc + lay.pix[0]), reinterpret_cast<uint32_t*>(sc + lay.pix[1])};
    int where = 0;                                             // 0: argb, 1 / 2: bufs[where - 1]
    for (int i = ntr - 1; i >= 0; --i) {
        const uint32_t* r = rec + TR_AT + TR_STRIDE * i;
        const int t = (int)r[0], b = (int)r[1], w = min((int)r[2], im.w);
        const uint32_t* data = reinterpret_cast<const uint32_t*>(sc + r[3]);
        const int n = w * h;                                   // <= im.w * im.h words of a scratch buffer
        uint32_t* dst = (t == 3 || where == 0) ? bufs[where == 1 ? 1 : 0] : bufs[where - 1];
        if (t == 0) {
            inverse_predictor(cur, dst, w, h, b, data, lane);
        } else if (t == 1) {
            const int bw = subsample(w, b);
            for (int k = lane; k < n; k += 64) {
                const int y = k / w, x = k - y * w;
                const uint32_t m = data[(y >> b) * bw + (x >> b)], v = cur[k];
                const int g2r = (int8_t)(m & 255), g2b = (int8_t)((m >> 8) & 255), r2b = (int8_t)((m >> 16) & 255);
                const int g = (int8_t)((v >> 8) & 255);
                const int red = (int)((v >> 16) & 255) + ((g2r * g) >> 5);
                int blue = (int)(v & 255) + ((g2b * g) >> 5);
                blue += (r2b * (int)(int8_t)(red & 255)) >> 5;
                dst[k] = (v & 0xFF00FF00u) | ((uint32_t)(red & 255) << 16) | (uint32_t)(blue & 255);
            }
        } else if (t == 2) {
            for (int k = lane; k < n; k += 64) {
                const uint32_t v = cur[k], g = (v >> 8) & 255;
                dst[k] = (v & 0xFF00FF00u) | ((((v >> 16) + g) & 255) << 16) | ((v + g) & 255);
            }
        } else {
            const int pn = min((int)r[4], 256), cw = subsample(w, b), per = (1 << b) - 1, nb = 8 >> b;
            for (int k = lane; k < n; k += 64) {
                const int y = k / w, x = k - y * w;
                const int idx = (int)(((cur[y * cw + (x >> b)] >> 8) & 255) >> ((x & per) * nb)) & ((1 << nb) - 1);
                dst[k] = idx < pn ? data[idx] : 0u;
            }
        }
        where = dst == bufs[0] ? 1 : 2;
        cur = dst;
        __threadfence_block();
        __syncthreads();
    }
    if (lane == 0) rec[2] = (uint32_t)where;
}

__global__ __launch_bounds__(256) void webp_convert_kernel(const maf_webp_image_t* images, const uint32_t* argb, const uint8_t* scratch, uint8_t* out,
                                                            const int32_t* status) {
    const maf_webp_image_t im = images[blockIdx.y];
    const int64_t npix = (int64_t)im.w * im.h;
    const int64_t q = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;      // the grid is sized by the largest image of the call
    if (q >= npix) return;
    const uint8_t* sc = scratch + im.scratch_off;
    const ScratchLayout lay = scratch_layout(im.w, im.h, im.dir_words, im.arena_units);
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(sc + lay.meta);
    const bool bad = status[blockIdx.y] != 0;
    const uint32_t where = bad ? 0u : rec[2];
    const uint32_t* src = where == 1 || where == 2 ? reinterpret_cast<const uint32_t*>(sc + lay.pix[where - 1]) : argb + im.argb_off;
    const int n = (int)min((int64_t)4, npix - q);
    uint8_t px[12];
    for (int j = 0; j < 4; ++j) {
        const uint32_t v = (j < n && !bad) ? src[q + j] : 0u;
        px[3 * j] = (uint8_t)v;
        px[3 * j + 1] = (uint8_t)(v >> 8);
        px[3 * j + 2] = (uint8_t)(v >> 16);
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

extern "C" int maf_webp_struct_sizes(int32_t* out) {
    WEBP_REQUIRE(out, "webp_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_webp_header_t); out[1] = (int32_t)sizeof(maf_webp_image_t);
    return 0;
}

extern "C" int maf_webp_decode(const void* blob_host, const void* blob_dev, uint32_t* argb, uint8_t* scratch, uint8_t* out, int32_t* status,
                               int32_t stages, maf_webp_stream_t stream) {
    WEBP_REQUIRE(blob_host && blob_dev && argb && scratch && out && status, "webp_decode: null pointer");
    WEBP_REQUIRE(stages > 0 && (stages & ~MAF_WEBP_STAGE_ALL) == 0, "webp_decode: stages is a mask of MAF_WEBP_STAGE_*");
    WEBP_REQUIRE(maf_aligned({blob_dev, argb, scratch, out}), "webp_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_webp_header_t hd = maf_blob_header<maf_webp_header_t>(hb);
    const int64_t T = hd.total_bytes;
    WEBP_REQUIRE(maf_blob_count_ok(hd.n_images), "webp_decode: 1 to 65535 images per call");
    WEBP_REQUIRE(maf_blob_size_ok(T), "webp_decode: blob size out of range");
    WEBP_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_webp_image_t), T) && in_blob(hd.stream_off, hd.stream_bytes, T) &&
                 hd.stream_bytes >= MAF_WEBP_STREAM_PAD && hd.stream_bytes % 8 == 0, "webp_decode: a blob section lies outside the blob");
    WEBP_REQUIRE(hd.argb_words > 0 && hd.scratch_bytes > 0 && hd.out_bytes > 0, "webp_decode: empty output buffers");
    const maf_webp_image_t* ims = reinterpret_cast<const maf_webp_image_t*>(hb + hd.images_off);
    const int64_t stream_data = hd.stream_bytes - MAF_WEBP_STREAM_PAD;
    int64_t max_quads = 1;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_webp_image_t& m = ims[i];
        WEBP_REQUIRE(m.w > 0 && m.h > 0 && m.w <= MAF_WEBP_MAX_SIDE && m.h <= MAF_WEBP_MAX_SIDE, "webp_decode: bad image size");
        const int64_t px = (int64_t)m.w * m.h;
        WEBP_REQUIRE(3 * px < ((int64_t)1 << 31), "webp_decode: an image of 2 GiB or more");
        WEBP_REQUIRE(m.stream_begin >= 0 && m.stream_begin <= m.stream_end && m.stream_end <= stream_data, "webp_decode: an image's stream lies outside the stream section");
        WEBP_REQUIRE(m.dir_words >= 40 && m.arena_units >= 64 && m.dir_words < (1 << 30) && m.arena_units < (1 << 30), "webp_decode: table space out of range");
        WEBP_REQUIRE(m.argb_off >= 0 && m.argb_off % 4 == 0 && m.argb_off <= hd.argb_words && px <= hd.argb_words - m.argb_off,
                     "webp_decode: an image's pixels lie outside the argb buffer");
        const ScratchLayout lay = scratch_layout(m.w, m.h, m.dir_words, m.arena_units);
        WEBP_REQUIRE(m.scratch_off >= 0 && m.scratch_off % 16 == 0 && m.scratch_bytes >= lay.total && m.scratch_off <= hd.scratch_bytes &&
                     m.scratch_bytes <= hd.scratch_bytes - m.scratch_off && lay.total < ((int64_t)1 << 32), "webp_decode: an image's scratch lies outside the scratch buffer");
        WEBP_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off <= hd.out_bytes && 3 * px <= hd.out_bytes - m.out_off,
                     "webp_decode: a frame lies outside the output buffer");
        const int64_t quads = (px + 3) / 4;
        max_quads = quads > max_quads ? quads : max_quads;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_webp_image_t* d_ims = reinterpret_cast<const maf_webp_image_t*>(db + hd.images_off);
    if (stages & MAF_WEBP_STAGE_ENTROPY) {
        const int rc = maf_check_hip(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s), "webp_decode memset");
        if (rc) return rc;
        hipLaunchKernelGGL(webp_entropy_kernel, dim3(hd.n_images), dim3(64), 0, s, d_ims, db + hd.stream_off, hd.stream_bytes, argb, scratch, status);
        const int rl = maf_check_hip(hipGetLastError(), "webp_entropy launch");
        if (rl) return rl;
    }
    if (stages & MAF_WEBP_STAGE_TRANSFORM) {
        hipLaunchKernelGGL(webp_transform_kernel, dim3(hd.n_images), dim3(64), 0, s, d_ims, argb, scratch, status);
        const int rl = maf_check_hip(hipGetLastError(), "webp_transform launch");
        if (rl) return rl;
    }
    if (stages & MAF_WEBP_STAGE_CONVERT) {
        hipLaunchKernelGGL(webp_convert_kernel, dim3((unsigned)((max_quads + 255) / 256), hd.n_images), dim3(256), 0, s, d_ims, argb, scratch, out, status);
        const int rl = maf_check_hip(hipGetLastError(), "webp_convert launch");
        if (rl) return rl;
    }
    return 0;
}
