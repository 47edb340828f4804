// zlib's trees.c (1.2.11) restated for ONE caller at a time (a lane of png_enc_block_kernel, or the host): build_tree, gen_bitlen, gen_codes,
// scan_tree / send_tree and the block type rule of _tr_flush_block.  Plain C++ over a work area the caller owns, so the same text compiles for
// the device and for the host.  The rules are written out in tests/png_encode_ref.py.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MAF_PNG_HD __host__ __device__ inline
#else
#define MAF_PNG_HD inline
#endif

namespace png_trees {

constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1, END_BLOCK = 256;
constexpr int STORED = 0, FIXED = 1, DYNAMIC = 2;
constexpr int HEAD_WORDS = 80, CODE_WORDS = 320;

struct Work {
    int32_t freq[HEAP_SIZE];             // in: the literal/length histogram in freq[0 .. 286)
    uint64_t heap[HEAP_SIZE + 1];        // frequency << 32 | depth << 16 | node: smaller() needs the heap's entries alone (one read, not three)
    uint16_t dad[HEAP_SIZE], len[HEAP_SIZE];
    uint8_t depth[HEAP_SIZE];
    uint8_t llen[L_CODES], dlen[D_CODES], bllen[BL_CODES];
    int32_t bl_count[16];
    uint16_t blcode[BL_CODES];
    int32_t opt_len, static_len;
};

struct Plan { int type, bits, head_bits; };

// trees.c _length_code / base_length / extra_lbits for a match length 3 .. 258
MAF_PNG_HD int len_code(int len) {
    if (len == 258) return 28;
    const int l = len - 3;
    if (l < 8) return l;
    int e = 0;                                               // groups of four codes with e = 1 .. 5 extra bits from l = 8 on
    for (int t = l >> 3; t; t >>= 1) ++e;
    return 4 * e + 4 + ((l >> e) & 3);
}
MAF_PNG_HD int len_extra(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
MAF_PNG_HD int len_base(int code) { return code < 8 ? code + 3 : code == 28 ? 258 : 3 + ((4 + (code & 3)) << len_extra(code)); }
MAF_PNG_HD int dist_extra(int code) { return code < 4 ? 0 : (code - 2) >> 1; }
MAF_PNG_HD int static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
MAF_PNG_HD uint32_t bit_reverse(uint32_t code, int len) {
    uint32_t r = 0;
    for (int i = 0; i < len; ++i, code >>= 1) r = (r << 1) | (code & 1u);
    return r;
}

enum Kind { LTREE, DTREE, BLTREE };

// trees.c smaller(): the lower frequency first, on a tie depth[n] <= depth[m] — one comparison of the packed heap entries without their node
MAF_PNG_HD uint64_t heap_entry(const Work& W, int n) { return ((uint64_t)(uint32_t)W.freq[n] << 32) | ((uint64_t)W.depth[n] << 16) | (uint64_t)n; }
MAF_PNG_HD bool smaller(uint64_t n, uint64_t m) { return (n >> 16) <= (m >> 16); }

MAF_PNG_HD void down_heap(Work& W, int heap_len, int k) {
    const uint64_t v = W.heap[k];
    int j = k << 1;
    while (j <= heap_len) {
        uint64_t c = W.heap[j];
        if (j < heap_len) {
            const uint64_t r = W.heap[j + 1];
            if (smaller(r, c)) { c = r; ++j; }
        }
        if (smaller(v, c)) break;
        W.heap[k] = c;
        k = j;
        j <<= 1;
    }
    W.heap[k] = v;
}

MAF_PNG_HD int xbits_of(Kind kind, int n) {
    if (kind == LTREE) return n >= 257 ? len_extra(n - 257) : 0;
    if (kind == DTREE) return dist_extra(n);
    return n == 16 ? 2 : n == 17 ? 3 : n == 18 ? 7 : 0;
}

// build_tree + gen_bitlen over W.freq[0 .. elems): the lengths are left in W.len[0 .. elems), opt_len / static_len are updated -> max_code
MAF_PNG_HD int build_tree(Work& W, Kind kind, int elems, int max_length) {
    int heap_len = 0, heap_max = HEAP_SIZE, max_code = -1;
    for (int n = 0; n < elems; ++n) {
        if (W.freq[n] != 0) {
            W.depth[n] = 0;
            W.heap[++heap_len] = heap_entry(W, max_code = n);
        } else {
            W.len[n] = 0;
        }
    }
    while (heap_len < 2) {
        const int node = max_code < 2 ? ++max_code : 0;
        W.freq[node] = 1;
        W.depth[node] = 0;
        W.heap[++heap_len] = heap_entry(W, node);
        W.opt_len--;
        if (kind == LTREE) W.static_len -= static_llen(node);
        if (kind == DTREE) W.static_len -= 5;
    }
    for (int n = heap_len / 2; n >= 1; --n) down_heap(W, heap_len, n);
    int node = elems;
    do {
        const int n = (int)(W.heap[1] & 0xFFFFu);
        W.heap[1] = W.heap[heap_len--];
        down_heap(W, heap_len, 1);
        const int m = (int)(W.heap[1] & 0xFFFFu);
        W.heap[--heap_max] = (uint64_t)n;                        // the sorted part holds bare nodes
        W.heap[--heap_max] = (uint64_t)m;
        W.freq[node] = W.freq[n] + W.freq[m];
        W.depth[node] = (uint8_t)((W.depth[n] >= W.depth[m] ? W.depth[n] : W.depth[m]) + 1);
        W.dad[n] = W.dad[m] = (uint16_t)node;
        W.heap[1] = heap_entry(W, node++);
        down_heap(W, heap_len, 1);
    } while (heap_len >= 2);
    W.heap[--heap_max] = W.heap[1] & 0xFFFFu;
    // gen_bitlen
    for (int b = 0; b < 16; ++b) W.bl_count[b] = 0;
    W.len[(int)W.heap[heap_max]] = 0;
    int overflow = 0;
    for (int h = heap_max + 1; h < HEAP_SIZE; ++h) {
        const int n = (int)W.heap[h];
        int bits = W.len[W.dad[n]] + 1;
        if (bits > max_length) { bits = max_length; ++overflow; }
        W.len[n] = (uint16_t)bits;
        if (n > max_code) continue;
        W.bl_count[bits]++;
        const int xbits = xbits_of(kind, n);
        W.opt_len += W.freq[n] * (bits + xbits);
        if (kind == LTREE) W.static_len += W.freq[n] * (static_llen(n) + xbits);
        if (kind == DTREE) W.static_len += W.freq[n] * (5 + xbits);
    }
    if (overflow > 0) {
        do {
            int bits = max_length - 1;
            while (W.bl_count[bits] == 0) --bits;
            W.bl_count[bits]--;
            W.bl_count[bits + 1] += 2;
            W.bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        int h = HEAP_SIZE;
        for (int bits = max_length; bits != 0; --bits) {
            int n = W.bl_count[bits];
            while (n != 0) {
                const int m = (int)W.heap[--h];
                if (m > max_code) continue;
                if (W.len[m] != bits) {
                    W.opt_len += (bits - (int)W.len[m]) * W.freq[m];
                    W.len[m] = (uint16_t)bits;
                }
                --n;
            }
        }
    }
    return max_code;
}

// gen_codes over lens[0 .. max_code]: emit(n, bit-reversed code, length) for every symbol with a code
template <typename Len, typename Emit>
MAF_PNG_HD void gen_codes(Len&& len_of, int max_code, Emit&& emit) {
    int count[16], next[16];
    for (int b = 0; b < 16; ++b) count[b] = 0;
    for (int n = 0; n <= max_code; ++n) count[len_of(n)]++;
    count[0] = 0;
    int code = 0;
    next[0] = 0;
    for (int b = 1; b < 16; ++b) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (int n = 0; n <= max_code; ++n) {
        const int l = len_of(n);
        if (l) emit(n, bit_reverse((uint32_t)next[l]++, l), l);
    }
}

// the loop scan_tree and send_tree share: emit(symbol of the bit-length alphabet, repeat count; 0 for a plain length)
template <typename Emit>
MAF_PNG_HD void walk_tree(const uint8_t* lens, int max_code, Emit&& emit) {
    int prevlen = -1, nextlen = lens[0], count = 0;
    int max_count = nextlen == 0 ? 138 : 7, min_count = nextlen == 0 ? 3 : 4;
    for (int n = 0; n <= max_code; ++n) {
        const int curlen = nextlen;
        nextlen = n + 1 <= max_code ? lens[n + 1] : 0xFFFF;      // the guard trees.c writes behind the last length
        if (++count < max_count && curlen == nextlen) continue;
        if (count < min_count) {
            for (int i = 0; i < count; ++i) emit(curlen, 0);
        } else if (curlen != 0) {
            if (curlen != prevlen) { emit(curlen, 0); --count; }
            emit(16, count);
        } else if (count <= 10) {
            emit(17, count);
        } else {
            emit(18, count);
        }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

// appends fields, least significant bit first, to a zeroed word array
struct HeadWriter {
    uint32_t* words;
    int n_words, bits;
    MAF_PNG_HD void put(uint32_t value, int nbits) {
        if (nbits == 0) return;
        const int w = bits >> 5, s = bits & 31;
        if (w < n_words) words[w] |= value << s;
        if (s + nbits > 32 && w + 1 < n_words) words[w + 1] |= value >> (32 - s);
        bits += nbits;
    }
};

// _tr_flush_block for one block.  W.freq[0 .. 286) holds the literal/length histogram WITHOUT end-of-block, n_match the matches (all at distance
// 1 = distance code 0), stored_len the bytes the block covers.  -> the plan; codes[CODE_WORDS] (length << 16 | code; 286 literal/length codes,
// then 30 distance codes) and head[HEAD_WORDS] (the 3 header bits, then the trees of a dynamic block) are written for every type.
MAF_PNG_HD Plan plan_block(Work& W, int n_match, int stored_len, bool last, uint32_t* codes, uint32_t* head) {
    const uint8_t bl_order[BL_CODES] ={16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    W.opt_len = W.static_len = 0;
    W.freq[END_BLOCK] = 1;
    const int lmax = build_tree(W, LTREE, L_CODES, 15);
    for (int n = 0; n < L_CODES; ++n) W.llen[n] = (uint8_t)W.len[n];
    for (int n = 0; n < D_CODES; ++n) W.freq[n] = 0;
    W.freq[0] = n_match;
    const int dmax = build_tree(W, DTREE, D_CODES, 15);
    for (int n = 0; n < D_CODES; ++n) W.dlen[n] = (uint8_t)W.len[n];
    for (int n = 0; n < BL_CODES; ++n) W.freq[n] = 0;
    walk_tree(W.llen, lmax, [&](int sym, int) { W.freq[sym]++; });
    walk_tree(W.dlen, dmax, [&](int sym, int) { W.freq[sym]++; });
    build_tree(W, BLTREE, BL_CODES, 7);
    for (int n = 0; n < BL_CODES; ++n) W.bllen[n] = (uint8_t)W.len[n];
    int max_blindex = BL_CODES - 1;
    for (; max_blindex >= 3; --max_blindex)
        if (W.bllen[bl_order[max_blindex]] != 0) break;
    W.opt_len += 3 * (max_blindex + 1) + 14;
    int opt_lenb = (W.opt_len + 3 + 7) >> 3;
    const int static_lenb = (W.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    for (int i = 0; i < HEAD_WORDS; ++i) head[i] = 0;
    for (int i = 0; i < CODE_WORDS; ++i) codes[i] = 0;
    HeadWriter hw = {head, HEAD_WORDS, 0};
    Plan p;
    if (stored_len + 4 <= opt_lenb) {
        p.type = STORED;
        p.bits = 3 + 32 + 8 * stored_len;
        hw.put((uint32_t)last, 3);
    } else if (static_lenb == opt_lenb) {
        p.type = FIXED;
        p.bits = 3 + W.static_len;
        hw.put((uint32_t)last | (1u << 1), 3);
        gen_codes([](int n) { return static_llen(n); }, 287, [&](int n, uint32_t c, int l) { if (n < L_CODES) codes[n] = ((uint32_t)l << 16) | c; });
        for (int n = 0; n < D_CODES; ++n) codes[L_CODES + n] = (5u << 16) | bit_reverse((uint32_t)n, 5);
    } else {
        p.type = DYNAMIC;
        p.bits = 3 + W.opt_len;
        hw.put((uint32_t)last | (2u << 1), 3);
        gen_codes([&](int n) { return (int)W.llen[n]; }, lmax, [&](int n, uint32_t c, int l) { codes[n] = ((uint32_t)l << 16) | c; });
        gen_codes([&](int n) { return (int)W.dlen[n]; }, dmax, [&](int n, uint32_t c, int l) { codes[L_CODES + n] = ((uint32_t)l << 16) | c; });
        gen_codes([&](int n) { return (int)W.bllen[n]; }, BL_CODES - 1, [&](int n, uint32_t c, int) { W.blcode[n] = (uint16_t)c; });
        hw.put((uint32_t)(lmax + 1 - 257), 5);
        hw.put((uint32_t)(dmax + 1 - 1), 5);
        hw.put((uint32_t)(max_blindex + 1 - 4), 4);
        for (int rank = 0; rank <= max_blindex; ++rank) hw.put(W.bllen[bl_order[rank]], 3);
        auto send = [&](int sym, int count) {
            hw.put(W.blcode[sym], W.bllen[sym]);
            if (sym == 16) hw.put((uint32_t)(count - 3), 2);
            if (sym == 17) hw.put((uint32_t)(count - 3), 3);
            if (sym == 18) hw.put((uint32_t)(count - 11), 7);
        };
        walk_tree(W.llen, lmax, send);
        walk_tree(W.dlen, dmax, send);
    }
    p.head_bits = hw.bits;
    return p;
}

}  // namespace png_trees
