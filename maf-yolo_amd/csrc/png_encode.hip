// PNG encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any row pitch), 8-bit RGB PNG files out
// whose zlib stream is, byte for byte, what zlib 1.2.11 writes at level 1, strategy Z_RLE, memLevel 8, window 15 (the settings cv2.imwrite
// hands libpng) over the filtered rows.  Replaces the final cv2.imwrite of Inferer.infer (yolov6/core/inferer.py) for a .png source.  The
// rules are restated in tests/png_encode_ref.py; the trees are csrc/png_trees.h; the host side (sizes, the job table) is
// maf-yolo_amd/png_encode.py; include/mafyolo_png_encode.h lists the ten kernels, the blob and the buffers.
//
// Every index that depends on pixel content (symbol counts, bit offsets, lengths) is bounded by construction (a symbol covers at least one
// byte; MAF_PNG_ENC_ZBOUND) and compared with its region's size before a store all the same.
#include "maf_common.h"
#include "../../include/mafyolo_png_encode.h"
#include "image_blob.h"
#include "block_scan.h"
#include "png_trees.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MAF_PNG_ENC_CHUNK;
constexpr int BSYM = MAF_PNG_ENC_BLOCK_SYMBOLS;
constexpr int NONE_AFTER = 0x7FFFFFFF;
constexpr int EMIT_ITEMS = 8;
constexpr uint32_t ADLER = 65521u, CRC_POLY = 0xEDB88320u;
static_assert(CHUNK == 16 * NT && CHUNK == 1 << 12, "a thread owns 16 bytes of a chunk; crc_x_pow_bytes_in_chunk takes 12 bits");
static_assert(MAF_PNG_ENC_CODE_WORDS == png_trees::CODE_WORDS && MAF_PNG_ENC_HEAD_WORDS == png_trees::HEAD_WORDS && BSYM == (1 << 14) - 1, "png_trees.h");
static_assert(MAF_PNG_ENC_STORED == png_trees::STORED && MAF_PNG_ENC_FIXED == png_trees::FIXED && MAF_PNG_ENC_DYNAMIC == png_trees::DYNAMIC, "block types");

// the last job whose first chunk or block is at most i
template <typename F>
__device__ __forceinline__ int job_of(int n, int i, F first) {
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

// exclusive scan of in[0 .. n) into out[0 .. n) by ONE workgroup (in == out is fine); returns the total
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

// ---- the filter (PNG 1.2, 6): the byte at position p of the file's filtered stream
__device__ __forceinline__ uint32_t filtered_byte(const maf_png_enc_job_t& j, int rowlen, int p) {
    const int y = p / rowlen, c = p - y * rowlen;
    if (c == 0) return (uint32_t)j.filter;
    const int px = (c - 1) / 3, ch = (c - 1) - 3 * px;
    const uint8_t* at = static_cast<const uint8_t*>(j.src) + (int64_t)y * j.pitch + 3 * px + 2 - ch;      // R, G, B in the file; B, G, R in the frame
    const int x = at[0];
    if (j.filter == 0) return (uint32_t)x;
    const int a = px > 0 ? at[-3] : 0;
    if (j.filter == 1) return (uint32_t)(x - a) & 255u;
    const int b = y > 0 ? at[-j.pitch] : 0;
    if (j.filter == 2) return (uint32_t)(x - b) & 255u;
    if (j.filter == 3) return (uint32_t)(x - ((a + b) >> 1)) & 255u;
    const int cc = px > 0 && y > 0 ? at[-j.pitch - 3] : 0;
    const int pa = abs(b - cc), pb = abs(a - cc), pc = abs(a + b - 2 * cc);
    return (uint32_t)(x - (pa <= pb && pa <= pc ? a : pb <= pc ? b : cc)) & 255u;
}

__device__ __forceinline__ uint32_t byte_of(const u32x4_t& v, int i) { return (v[i >> 2] >> (8 * (i & 3))) & 0xFFu; }

// chunks: int32 [5][n_chunks]: last run start in the chunk (-1), first (NONE_AFTER), last before the chunk, first behind it, symbols (then: first symbol)
__global__ __launch_bounds__(NT) void png_enc_filter_kernel(const maf_png_enc_job_t* jobs, int n_files, int n_chunks, uint8_t* raw, int32_t* chunks,
                                                             unsigned long long* sums) {
    __shared__ unsigned int sh_a;
    __shared__ unsigned long long sh_b;
    __shared__ int sh_last, sh_first;
    const int ch = blockIdx.x;
    const int f = job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; });
    const maf_png_enc_job_t j = jobs[f];
    if (threadIdx.x == 0) { sh_a = 0u; sh_b = 0ull; sh_last = -1; sh_first = NONE_AFTER; }
    __syncthreads();
    const int64_t p0 = (int64_t)(ch - j.chunk0) * CHUNK + 16 * threadIdx.x;
    if (p0 < j.n_raw) {
        const int rowlen = 1 + 3 * j.w, n = j.n_raw, q0 = (int)p0;
        uint32_t prev = q0 > 0 ? filtered_byte(j, rowlen, q0 - 1) : 0x100u;      // 0x100: no byte equals it, byte 0 starts a run
        uint32_t a = 0u, b = 0u, w[4] = {0u, 0u, 0u, 0u};
        int last = -1, first = NONE_AFTER;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = q0 + i;
            if (p < n) {
                const uint32_t v = filtered_byte(j, rowlen, p);
                w[i >> 2] |= v << (8 * (i & 3));
                a += v;
                b += v * ((uint32_t)(n - p) % ADLER);                            // 16 * 255 * 65520 < 2^32
                if (v != prev) {
                    last = p;
                    if (first == NONE_AFTER) first = p;
                }
                prev = v;
            }
        }
        const u32x4_t v = {w[0], w[1], w[2], w[3]};
        *reinterpret_cast<u32x4_t*>(raw + j.raw_off + q0) = v;                    // the file's region is a multiple of 16 bytes
        atomicAdd(&sh_a, a);
        atomicAdd(&sh_b, (unsigned long long)b);
        if (last >= 0) { atomicMax(&sh_last, last); atomicMin(&sh_first, first); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        chunks[ch] = sh_last;
        chunks[n_chunks + ch] = sh_first;
        if (sh_a) {
            atomicAdd(&sums[4 * f], (unsigned long long)sh_a);                   // sums of bytes below 2^31 * 255: no overflow
            atomicAdd(&sums[4 * f + 1], sh_b % ADLER);
        }
    }
}

__global__ __launch_bounds__(NT) void png_enc_runs_kernel(const maf_png_enc_job_t* jobs, int n_chunks, int32_t* chunks) {
    __shared__ int sh[NT];
    const maf_png_enc_job_t j = jobs[blockIdx.x];
    const int32_t* last = chunks + j.chunk0;
    const int32_t* first = chunks + n_chunks + j.chunk0;
    int32_t* before = chunks + 2 * n_chunks + j.chunk0;
    int32_t* after = chunks + 3 * n_chunks + j.chunk0;
    int carry = -1;
    for (int t0 = 0; t0 < j.n_chunks; t0 += NT) {                                // forward: the last run start before each chunk
        const int i = t0 + threadIdx.x;
        const int v = i < j.n_chunks ? last[i] : -1;
        const int ex = max(carry, block_excl_scan(v, -1, (int)threadIdx.x, sh, [](int x, int y) { return max(x, y); }));
        if (i < j.n_chunks) before[i] = ex;
        if (threadIdx.x == NT - 1) sh[0] = max(ex, v);
        __syncthreads();
        carry = sh[0];
        __syncthreads();
    }
    carry = j.n_raw;
    for (int t0 = 0; t0 < j.n_chunks; t0 += NT) {                                // backward: the first run start behind each chunk (n_raw: none)
        const int i = j.n_chunks - 1 - (t0 + (int)threadIdx.x);
        const int v = i >= 0 ? first[i] : NONE_AFTER;
        const int ex = min(carry, block_excl_scan(v, NONE_AFTER, (int)threadIdx.x, sh, [](int x, int y) { return min(x, y); }));
        if (i >= 0) after[i] = ex;
        if (threadIdx.x == NT - 1) sh[0] = min(ex, v);
        __syncthreads();
        carry = sh[0];
        __syncthreads();
    }
}

// The run rule.  A position p of a run [ps, pe) starts a symbol when it is the run's first byte (a literal), or with k = p - ps - 1, r = pe - ps - 1,
// q = r / 258, rem = r % 258: k < 258 q and k % 258 == 0 (a match of 258), k == 258 q and rem >= 3 (a match of rem), k >= 258 q and rem < 3 (a literal).
template <bool WRITE>
__global__ __launch_bounds__(NT) void png_enc_tokens_kernel(const maf_png_enc_job_t* jobs, int n_files, int n_chunks, const uint8_t* raw, int32_t* chunks,
                                                             uint16_t* tok, maf_png_enc_block_t* blocks) {
    __shared__ int sh[NT];
    const int ch = blockIdx.x;
    const maf_png_enc_job_t j = jobs[job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; })];
    const int64_t p64 = (int64_t)(ch - j.chunk0) * CHUNK + 16 * threadIdx.x;
    const int n = j.n_raw;
    const bool live = p64 < n;
    const int p0 = live ? (int)p64 : n;
    u32x4_t v = {0u, 0u, 0u, 0u};
    uint32_t starts = 0u;                                                       // bit i: byte p0 + i starts a run
    if (live) {
        v = *reinterpret_cast<const u32x4_t*>(raw + j.raw_off + p0);
        uint32_t prev = p0 > 0 ? raw[j.raw_off + p0 - 1] : 0x100u;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t b = byte_of(v, i);
            if (p0 + i < n && b != prev) starts |= 1u << i;
            prev = b;
        }
    }
    const int mine_last = starts ? p0 + 31 - __clz(starts) : -1, mine_first = starts ? p0 + __ffs(starts) - 1 : NONE_AFTER;
    int ps = max(chunks[2 * n_chunks + ch], block_excl_scan(mine_last, -1, (int)threadIdx.x, sh, [](int x, int y) { return max(x, y); }));
    const int behind = min(chunks[3 * n_chunks + ch], block_excl_scan(mine_first, NONE_AFTER, NT - 1 - (int)threadIdx.x, sh, [](int x, int y) { return min(x, y); }));
    uint32_t symbols = 0u;                                                      // bit i: byte p0 + i starts a symbol
    uint32_t lens[16];
    if (live) {
        int pe = behind;
        int ends[16];
#pragma unroll
        for (int i = 15; i >= 0; --i) {
            ends[i] = pe;
            if ((starts >> i) & 1u) pe = p0 + i;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int p = p0 + i;
            lens[i] = 0u;
            if (p >= n) continue;
            if ((starts >> i) & 1u) {
                ps = p;
                symbols |= 1u << i;
                continue;
            }
            const int k = p - ps - 1, r = ends[i] - ps - 1, q = r / 258, rem = r - 258 * q;
            if (k < 258 * q) {
                if (k % 258 == 0) { symbols |= 1u << i; lens[i] = 258u; }
            } else if (rem >= 3) {
                if (k == 258 * q) { symbols |= 1u << i; lens[i] = (uint32_t)rem; }
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
    for (int i = 0; i < 16; ++i) {
        if (!((symbols >> i) & 1u)) continue;
        if (idx < n) {                                                           // always: a symbol covers at least one byte
            tok[j.raw_off + idx] = (uint16_t)(lens[i] ? 256u + lens[i] : byte_of(v, i));
            if (idx % BSYM == 0) blocks[j.block0 + idx / BSYM].pos = p0 + i;
        }
        ++idx;
    }
}

__global__ __launch_bounds__(NT) void png_enc_symscan_kernel(const maf_png_enc_job_t* jobs, int n_chunks, int32_t* chunks, unsigned long long* sums,
                                                              maf_png_enc_block_t* blocks) {
    __shared__ int64_t sh[NT];
    const maf_png_enc_job_t j = jobs[blockIdx.x];
    int32_t* c = chunks + 4 * n_chunks + j.chunk0;
    const int64_t total = scan_by_one_workgroup(c, nullptr, c, j.n_chunks, sh);
    if (threadIdx.x == 0) {
        sums[4 * blockIdx.x + 3] = (unsigned long long)total;
        if (total % BSYM == 0 && total / BSYM < j.n_blocks) blocks[j.block0 + total / BSYM].pos = j.n_raw;      // the empty last block
    }
}

__global__ __launch_bounds__(64) void png_enc_block_kernel(const maf_png_enc_job_t* jobs, int n_files, const uint16_t* tok, const unsigned long long* sums,
                                                            maf_png_enc_block_t* blocks, uint32_t* codes, uint32_t* heads) {
    __shared__ png_trees::Work W;
    __shared__ int n_match;
    const int b = blockIdx.x;
    const int f = job_of(n_files, b, [&](int i) { return jobs[i].block0; });
    const maf_png_enc_job_t j = jobs[f];
    const int k = b - j.block0;
    const int64_t total = (int64_t)sums[4 * f + 3];
    const int nb = (int)(total / BSYM) + 1;
    maf_png_enc_block_t* blk = blocks + b;
    if (k >= nb) {
        if (threadIdx.x == 0) {
            blk->bitoff = 0; blk->pos = j.n_raw; blk->type = MAF_PNG_ENC_UNUSED; blk->bits = 0; blk->head_bits = 0; blk->n_sym = 0; blk->stored_len = 0;
        }
        return;
    }
    const int n_sym = (int)min((int64_t)BSYM, total - (int64_t)k * BSYM);
    for (int i = threadIdx.x; i < png_trees::L_CODES; i += 64) W.freq[i] = 0;
    if (threadIdx.x == 0) n_match = 0;
    __syncthreads();
    const uint16_t* t = tok + j.raw_off + (int64_t)k * BSYM;
    for (int i = threadIdx.x; i < n_sym; i += 64) {
        const int s = t[i];
        if (s < 256) {
            atomicAdd(&W.freq[s], 1);
        } else {
            atomicAdd(&W.freq[257 + png_trees::len_code(s - 256)], 1);
            atomicAdd(&n_match, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int pos = min(max(blk->pos, 0), j.n_raw), end = min(max(k + 1 < nb ? blk[1].pos : j.n_raw, pos), j.n_raw);      // in range whatever was read
        const png_trees::Plan p = png_trees::plan_block(W, n_match, end - pos, k == nb - 1, codes + (int64_t)b * MAF_PNG_ENC_CODE_WORDS,
                                                        heads + (int64_t)b * MAF_PNG_ENC_HEAD_WORDS);
        blk->type = p.type; blk->bits = p.bits; blk->head_bits = p.head_bits; blk->n_sym = n_sym; blk->stored_len = end - pos;
    }
}

__global__ __launch_bounds__(NT) void png_enc_offsets_kernel(const maf_png_enc_job_t* jobs, int n_files, const unsigned long long* sums, maf_png_enc_block_t* blocks,
                                                              int32_t* lengths, int64_t* offsets) {
    __shared__ int64_t sh[NT];
    for (int f = threadIdx.x; f < n_files; f += NT) {
        const maf_png_enc_job_t j = jobs[f];
        const int nb = (int)((int64_t)sums[4 * f + 3] / BSYM) + 1;
        int64_t at = 16;
        for (int k = 0; k < nb && k < j.n_blocks; ++k) {
            maf_png_enc_block_t* blk = blocks + j.block0 + k;
            blk->bitoff = at;
            if (blk->type == MAF_PNG_ENC_STORED) blk->bits += (int)((-(at + 3)) & 7);      // _tr_stored_block: bi_windup behind the 3 header bits
            at += blk->bits;
        }
        const int64_t zlen = min(((at + 7) >> 3) + 4, j.packed_bytes);          // never binds (MAF_PNG_ENC_ZBOUND)
        lengths[f] = (int32_t)(MAF_PNG_ENC_FILE_BYTES + zlen);
    }
    __syncthreads();
    scan_by_one_workgroup(lengths, offsets, nullptr, n_files, sh);
}

// ors the low `nbits` (at most 33) bits of `value` into the packed words at bit `at`
__device__ __forceinline__ void or_bits(uint32_t* words, int64_t n_words, int64_t at, uint64_t value) {
    const int64_t w = at >> 5;
    const uint64_t x = value << (at & 31);
    if ((uint32_t)x && w < n_words) atomicOr(words + w, (uint32_t)x);
    if ((uint32_t)(x >> 32) && w + 1 < n_words) atomicOr(words + w + 1, (uint32_t)(x >> 32));
}

__global__ __launch_bounds__(NT) void png_enc_emit_kernel(const maf_png_enc_job_t* jobs, int n_files, const uint8_t* raw, const uint16_t* tok,
                                                           const maf_png_enc_block_t* blocks, const uint32_t* codes, const uint32_t* heads, uint8_t* packed) {
    __shared__ uint32_t code[MAF_PNG_ENC_CODE_WORDS];
    __shared__ int sh[NT];
    __shared__ int tile_bits;
    const int b = blockIdx.x;
    const maf_png_enc_block_t blk = blocks[b];
    if (blk.type == MAF_PNG_ENC_UNUSED) return;
    const maf_png_enc_job_t j = jobs[job_of(n_files, b, [&](int i) { return jobs[i].block0; })];
    uint32_t* words = reinterpret_cast<uint32_t*>(packed + j.packed_off);
    const int64_t n_words = j.packed_bytes >> 2;
    for (int i = threadIdx.x; 32 * i < blk.head_bits && i < MAF_PNG_ENC_HEAD_WORDS; i += NT)
        or_bits(words, n_words, blk.bitoff + 32 * i, heads[(int64_t)b * MAF_PNG_ENC_HEAD_WORDS + i]);
    if (blk.type == MAF_PNG_ENC_STORED) {                                        // LEN, NLEN and the bytes, from the next byte boundary on
        const int64_t first = (blk.bitoff + 3 + 7) >> 3, end = first + 4 + blk.stored_len;
        const uint32_t len4 = ((uint32_t)blk.stored_len & 0xFFFFu) | ((~(uint32_t)blk.stored_len & 0xFFFFu) << 16);
        const uint8_t* src = raw + j.raw_off + min(max(blk.pos, 0), j.n_raw - blk.stored_len);      // stored_len is 0 .. n_raw
        for (int64_t w = (first >> 2) + threadIdx.x; 4 * w < end; w += NT) {
            uint32_t x = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t at = 4 * w + i - first;
                if (at >= 0 && at < 4) x |= ((len4 >> (8 * at)) & 0xFFu) << (8 * i);
                else if (at >= 4 && at < 4 + blk.stored_len) x |= (uint32_t)src[at - 4] << (8 * i);
            }
            if (w >= n_words) continue;
            if (4 * w >= first && 4 * w + 4 <= end) words[w] = x; else if (x) atomicOr(words + w, x);      // a word shared with a neighbour block is or-ed
        }
        return;
    }
    for (int i = threadIdx.x; i < MAF_PNG_ENC_CODE_WORDS; i += NT) code[i] = codes[(int64_t)b * MAF_PNG_ENC_CODE_WORDS + i];
    __syncthreads();
    const uint32_t dist = code[png_trees::L_CODES];                              // distance 1: distance code 0, no extra bits
    const int k = b - j.block0;
    const uint16_t* t = tok + j.raw_off + (int64_t)k * BSYM;
    int64_t at = blk.bitoff + blk.head_bits;
    for (int t0 = 0; t0 < blk.n_sym; t0 += NT * EMIT_ITEMS) {                    // a thread owns EMIT_ITEMS symbols in a row: one scan per tile, few words per thread
        const int i0 = t0 + EMIT_ITEMS * threadIdx.x;
        uint32_t bits[EMIT_ITEMS];
        int nbits[EMIT_ITEMS], ndist[EMIT_ITEMS], total = 0;
#pragma unroll
        for (int e = 0; e < EMIT_ITEMS; ++e) {
            bits[e] = 0u; nbits[e] = 0; ndist[e] = 0;
            if (i0 + e < blk.n_sym) {
                const int s = t[i0 + e];
                if (s < 256) {
                    bits[e] = code[s] & 0xFFFFu; nbits[e] = (int)(code[s] >> 16);
                } else {
                    const int lc = png_trees::len_code(s - 256);
                    const uint32_t c = code[257 + lc];
                    bits[e] = (c & 0xFFFFu) | ((uint32_t)(s - 256 - png_trees::len_base(lc)) << (c >> 16));      // at most 15 + 5 bits
                    nbits[e] = (int)(c >> 16) + png_trees::len_extra(lc);
                    ndist[e] = (int)(dist >> 16);
                }
            }
            total += nbits[e] + ndist[e];
        }
        const int before = block_excl_sum<NT>(total, sh);
        int64_t word = (at + before) >> 5;
        int fill = (int)((at + before) & 31);
        uint64_t acc = 0;                                                        // the bits gathered for `word`, from bit `fill` of it on
        bool shared = true;                                                      // the first word may hold the end of the thread before
        auto put = [&](uint32_t value, int n) {                                  // n <= 20, fill <= 31
            acc |= (uint64_t)value << fill;
            fill += n;
            if (fill >= 32) {
                if (word < n_words) {
                    if (shared) atomicOr(words + word, (uint32_t)acc); else words[word] = (uint32_t)acc;
                }
                shared = false;
                acc >>= 32;
                fill -= 32;
                ++word;
            }
        };
#pragma unroll
        for (int e = 0; e < EMIT_ITEMS; ++e) {
            if (nbits[e]) put(bits[e], nbits[e]);
            if (ndist[e]) put(dist & 0xFFFFu, ndist[e]);
        }
        if (fill > 0 && word < n_words) atomicOr(words + word, (uint32_t)acc);  // shared with the thread behind
        if (threadIdx.x == NT - 1) tile_bits = before + total;
        __syncthreads();
        at += tile_bits;
        __syncthreads();
    }
    if (threadIdx.x == 0) or_bits(words, n_words, at, code[png_trees::END_BLOCK] & 0xFFFFu);
}

// ---- CRC-32 (reflected, polynomial 0xEDB88320), zlib's crc32_combine by polynomial arithmetic: a(x) * b(x) mod P, x^0 = 0x80000000
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0u;
    for (uint32_t m = 0x80000000u; m; m >>= 1) {
        if (a & m) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_x_pow_bytes(int64_t n) {                 // x^(8 n) mod P
    uint32_t r = 0x80000000u, base = 0x00800000u;                                // 1, x^8
    for (; n; n >>= 1) {
        if (n & 1) r = crc_mul(base, r);
        base = crc_mul(base, base);
    }
    return r;
}
// x^(8 n) mod P for n below 4096 (a thread's distance to its chunk's end): the product of the x^(8 * 2^k) of its set bits, 6 multiplications on average
__device__ __forceinline__ uint32_t crc_x_pow_bytes_in_chunk(int n) {
    const uint32_t power[12] = {0x00800000u, 0x00008000u, 0xEDB88320u, 0xB1E6B092u, 0xA06A2517u, 0xED627DAEu,
                                0x88D14467u, 0xD7BBFE6Au, 0xEC447F11u, 0x8E7EA170u, 0x6427800Eu, 0x4D47BAE0u};      // x^8 squared k times
    uint32_t r = 0x80000000u;
#pragma unroll
    for (int k = 0; k < 12; ++k)
        if ((n >> k) & 1) r = crc_mul(power[k], r);
    return r;
}
__device__ __forceinline__ uint32_t crc_byte(uint32_t c, uint32_t byte) {
    c ^= byte;
#pragma unroll
    for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    return c;
}

__device__ __forceinline__ uint32_t adler_of(const maf_png_enc_job_t& j, const unsigned long long* s) {
    const uint32_t a = (uint32_t)((1ull + s[0]) % ADLER), b = (uint32_t)(((unsigned long long)j.n_raw + s[1]) % ADLER);
    return (b << 16) | a;
}

__global__ __launch_bounds__(NT) void png_enc_copy_kernel(const maf_png_enc_job_t* jobs, int n_files, const uint8_t* packed, unsigned long long* sums,
                                                           const int32_t* lengths, const int64_t* offsets, uint8_t* out, int64_t out_bytes) {
    __shared__ unsigned int sh_crc;
    __shared__ uint32_t stage[CHUNK / 4];
    const int ch = blockIdx.x;
    const int f = job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; });
    const maf_png_enc_job_t j = jobs[f];
    const int64_t zlen = lengths[f] - MAF_PNG_ENC_FILE_BYTES, first = (int64_t)(ch - j.chunk0) * CHUNK;
    if (first >= zlen) return;                                                   // the whole workgroup
    const int64_t chunk_end = min(first + CHUNK, zlen);
    if (threadIdx.x == 0) sh_crc = 0u;
    __syncthreads();
    const int64_t s0 = first + 16 * threadIdx.x;
    if (s0 < zlen) {
        const int valid = (int)min(zlen - s0, (int64_t)16);
        u32x4_t v = {0u, 0u, 0u, 0u};
        if (s0 + 16 <= j.packed_bytes) v = *reinterpret_cast<const u32x4_t*>(packed + j.packed_off + s0);
        const uint32_t adler = adler_of(j, sums + 4 * f);
        uint32_t c = 0xFFFFFFFFu, w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            if (i < valid) {
                const int64_t tail = s0 + i - (zlen - 4);
                const uint32_t byte = s0 + i < 2 ? (s0 + i == 0 ? 0x78u : 0x01u) : tail >= 0 ? (adler >> (8 * (3 - tail))) & 0xFFu : byte_of(v, i);
                w[i >> 2] |= byte << (8 * (i & 3));
                c = crc_byte(c, byte);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) stage[4 * threadIdx.x + i] = w[i];
        atomicXor(&sh_crc, crc_mul(~c, crc_x_pow_bytes_in_chunk((int)(chunk_end - s0 - valid))));      // moved to the chunk's end
    }
    __syncthreads();
    if (threadIdx.x == 0 && sh_crc) atomicXor(&sums[4 * f + 2], (unsigned long long)crc_mul(sh_crc, crc_x_pow_bytes(zlen - chunk_end)));
    // the chunk's bytes go out as aligned words (the file starts wherever the one before ended); the words at the chunk's two ends, which it
    // shares with its neighbours or with the frame of the file, byte by byte
    const uint8_t* bytes = reinterpret_cast<const uint8_t*>(stage);
    const int64_t o0 = offsets[f] + 41 + first;                                  // signature 8, IHDR 25, IDAT length and type 8
    const int len = (int)(chunk_end - first);
    for (int64_t a = (o0 & ~(int64_t)3) + 4 * threadIdx.x; a < o0 + len; a += 4 * NT) {
        const int rel = (int)(a - o0);
        if (rel >= 0 && rel + 4 <= len) {
            if (a + 4 <= out_bytes) *reinterpret_cast<uint32_t*>(out + a) = bytes[rel] | (bytes[rel + 1] << 8) | (bytes[rel + 2] << 16) | ((uint32_t)bytes[rel + 3] << 24);
        } else {
            for (int i = 0; i < 4; ++i)
                if (rel + i >= 0 && rel + i < len && a + i < out_bytes) out[a + i] = bytes[rel + i];
        }
    }
}

__global__ __launch_bounds__(NT) void png_enc_frame_kernel(const maf_png_enc_job_t* jobs, int n_files, const unsigned long long* sums, const int32_t* lengths,
                                                            const int64_t* offsets, uint8_t* out, int64_t out_bytes) {
    const int f = blockIdx.x * NT + threadIdx.x;
    if (f >= n_files) return;
    const maf_png_enc_job_t j = jobs[f];
    const int64_t zlen = lengths[f] - MAF_PNG_ENC_FILE_BYTES;
    int64_t o = offsets[f];
    uint32_t c = 0xFFFFFFFFu;
    auto put = [&](uint32_t byte) {
        if (o < out_bytes) out[o] = (uint8_t)byte;
        c = crc_byte(c, byte & 0xFFu);
        ++o;
    };
    auto put32 = [&](uint32_t x) { put(x >> 24); put((x >> 16) & 0xFFu); put((x >> 8) & 0xFFu); put(x & 0xFFu); };
    const uint32_t sig[2] = {0x89504E47u, 0x0D0A1A0Au};
    put32(sig[0]); put32(sig[1]);
    put32(13u);
    c = 0xFFFFFFFFu;
    put32(0x49484452u);                                                          // IHDR
    put32((uint32_t)j.w); put32((uint32_t)j.h);
    put(8u); put(2u); put(0u); put(0u); put(0u);
    put32(~c);
    put32((uint32_t)zlen);
    c = 0xFFFFFFFFu;
    put32(0x49444154u);                                                          // IDAT
    const uint32_t crc = crc_mul(~c, crc_x_pow_bytes(zlen)) ^ (uint32_t)sums[4 * f + 2];
    o += zlen;
    put32(crc);
    put32(0u);
    c = 0xFFFFFFFFu;
    put32(0x49454E44u);                                                          // IEND
    put32(~c);
}

}  // namespace

extern "C" int maf_png_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "png_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_png_enc_header_t); out[1] = (int32_t)sizeof(maf_png_enc_job_t); out[2] = (int32_t)sizeof(maf_png_enc_block_t);
    return 0;
}

extern "C" int maf_png_encode(const void* blob_host, const void* blob_dev, uint8_t* raw, uint16_t* tok, int32_t* chunks, uint64_t* sums, void* blocks, uint32_t* codes,
                              uint32_t* heads, uint8_t* packed, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_png_enc_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && raw && tok && chunks && sums && blocks && codes && heads && packed && out && lengths && offsets, "png_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, raw, packed}) && maf_aligned({sums, blocks, offsets}, 8) && maf_aligned({out}, 4),
                "png_encode: blob, raw and packed must be 16-byte aligned, the 64-bit buffers 8-byte aligned, out 4-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_png_enc_header_t hd = maf_blob_header<maf_png_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files), "png_encode: 1 to 65535 files per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "png_encode: blob size out of range");
    MAF_REQUIRE(hd.n_chunks > 0 && hd.n_chunks < (1 << 30) && hd.n_blocks > 0 && hd.n_blocks < (1 << 30), "png_encode: chunk or block count out of range");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(maf_png_enc_job_t), T), "png_encode: the job table lies outside the blob");
    const maf_png_enc_job_t* jobs = reinterpret_cast<const maf_png_enc_job_t*>(hb + hd.jobs_off);
    int64_t chunk = 0, block = 0, at_raw = 0, at_packed = 0, need = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const maf_png_enc_job_t& j = jobs[i];
        MAF_REQUIRE(j.src, "png_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= 65535 && j.h <= 65535, "png_encode: width and height are 1 to 65535");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "png_encode: a row pitch below 3 * width");
        MAF_REQUIRE(j.filter >= 0 && j.filter <= 4, "png_encode: a filter type outside 0..4");
        const int64_t n = (int64_t)j.h * (1 + 3 * (int64_t)j.w);
        MAF_REQUIRE(n < ((int64_t)1 << 31) && j.n_raw == n, "png_encode: n_raw is h * (1 + 3 * w), below 2 GiB");
        const int64_t bound = MAF_PNG_ENC_ZBOUND(n);
        MAF_REQUIRE(j.raw_off == at_raw && j.packed_off == at_packed, "png_encode: the files' regions must follow each other without gaps");
        MAF_REQUIRE((j.packed_bytes & 15) == 0 && j.packed_bytes >= bound, "png_encode: a packed region below the bound or not a multiple of 16");
        MAF_REQUIRE(j.n_chunks == (j.packed_bytes + CHUNK - 1) / CHUNK && j.chunk0 == chunk, "png_encode: the files' chunks must follow each other, sized by the bound");
        MAF_REQUIRE(j.n_blocks == n / BSYM + 1 && j.block0 == block, "png_encode: the files' blocks must follow each other, sized by the worst case");
        chunk += j.n_chunks;
        block += j.n_blocks;
        at_raw += (n + 15) / 16 * 16;
        at_packed += j.packed_bytes;
        need += MAF_PNG_ENC_FILE_BYTES + bound;
    }
    MAF_REQUIRE(chunk == hd.n_chunks && block == hd.n_blocks, "png_encode: the header's chunk or block count differs from the jobs' sum");
    MAF_REQUIRE(hd.raw_bytes >= at_raw && hd.packed_bytes >= at_packed && hd.out_bytes >= need, "png_encode: a device buffer is smaller than the worst case");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_png_enc_job_t* d_jobs = reinterpret_cast<const maf_png_enc_job_t*>(db + hd.jobs_off);
    maf_png_enc_block_t* d_blocks = static_cast<maf_png_enc_block_t*>(blocks);
    unsigned long long* d_sums = reinterpret_cast<unsigned long long*>(sums);
    int rc = maf_check_hip(hipMemsetAsync(packed, 0, (size_t)at_packed, s), "png_encode memset packed");
    if (rc) return rc;
    rc = maf_check_hip(hipMemsetAsync(sums, 0, (size_t)hd.n_files * 4 * sizeof(uint64_t), s), "png_encode memset sums");
    if (rc) return rc;
    hipLaunchKernelGGL(png_enc_filter_kernel, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_chunks, raw, chunks, d_sums);
    MAF_LAUNCH_CHECK("png_enc_filter");
    hipLaunchKernelGGL(png_enc_runs_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, hd.n_chunks, chunks);
    MAF_LAUNCH_CHECK("png_enc_runs");
    hipLaunchKernelGGL(png_enc_tokens_kernel<false>, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_chunks, raw, chunks, tok, d_blocks);
    MAF_LAUNCH_CHECK("png_enc_tokens (count)");
    hipLaunchKernelGGL(png_enc_symscan_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, hd.n_chunks, chunks, d_sums, d_blocks);
    MAF_LAUNCH_CHECK("png_enc_symscan");
    hipLaunchKernelGGL(png_enc_tokens_kernel<true>, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_chunks, raw, chunks, tok, d_blocks);
    MAF_LAUNCH_CHECK("png_enc_tokens (write)");
    hipLaunchKernelGGL(png_enc_block_kernel, dim3(hd.n_blocks), dim3(64), 0, s, d_jobs, hd.n_files, tok, d_sums, d_blocks, codes, heads);
    MAF_LAUNCH_CHECK("png_enc_block");
    hipLaunchKernelGGL(png_enc_offsets_kernel, dim3(1), dim3(NT), 0, s, d_jobs, hd.n_files, d_sums, d_blocks, lengths, offsets);
    MAF_LAUNCH_CHECK("png_enc_offsets");
    hipLaunchKernelGGL(png_enc_emit_kernel, dim3(hd.n_blocks), dim3(NT), 0, s, d_jobs, hd.n_files, raw, tok, d_blocks, codes, heads, packed);
    MAF_LAUNCH_CHECK("png_enc_emit");
    hipLaunchKernelGGL(png_enc_copy_kernel, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, packed, d_sums, lengths, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("png_enc_copy");
    hipLaunchKernelGGL(png_enc_frame_kernel, dim3((hd.n_files + NT - 1) / NT), dim3(NT), 0, s, d_jobs, hd.n_files, d_sums, lengths, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("png_enc_frame");
    return 0;
}
