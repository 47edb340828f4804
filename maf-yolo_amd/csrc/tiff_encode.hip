// TIFF encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any row pitch), 8-bit RGB TIFF files out
// whose strips are, byte for byte, what libtiff 4.7.1 writes at Compression 5 (LZW), Predictor 2, PlanarConfiguration 1 for the same rows (the
// settings cv2.imwrite hands it).  Replaces the final cv2.imwrite of Inferer.infer (yolov6/core/inferer.py) for a .tif / .tiff source.  The
// rules are restated in tests/tiff_encode_ref.py; the host side (sizes, the job table) is maf-yolo_amd/tiff_encode.py;
// include/mafyolo_tiff_encode.h lists the six kernels, the blob and the buffers.
//
// Every index that depends on pixel content (code counts, bit offsets, lengths) is bounded by construction (MAF_TIFF_ENC_CODE_BOUND) and
// compared with its region's size before a store all the same.
#include "maf_common.h"
#include "../../include/mafyolo_tiff_encode.h"
#include "image_blob.h"
#include "block_scan.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MAF_TIFF_ENC_CHUNK;
constexpr int TABLE = MAF_TIFF_ENC_TABLE;
constexpr int TILE = 1024;                   // input bytes the wave fetches at a time: 16 per lane
constexpr int CODE_CAP = TILE + 8;           // codes one pass of the walk can add: one per byte and one Clear
constexpr int PACK_ITEMS = 8;
constexpr uint32_t CLEAR = 256u, EOI = 257u, FIRST = 258u, TABLE_FULL = 4094u, CHECK_GAP = 10000u;
static_assert(CHUNK == 16 * NT, "a thread of the rows kernel owns 16 bytes of a chunk");
static_assert(TILE == 16 * 64 && (TABLE & (TABLE - 1)) == 0 && TABLE % 256 == 0, "the wave's tile and table");

// the last job whose first chunk or strip is at most i
template <typename F>
__device__ __forceinline__ int job_of(int n, int i, F first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive scan of in(i), i in [0, n), by ONE workgroup; put(i, sum before i); returns the total
template <typename In, typename Put>
__device__ __forceinline__ int64_t scan_by_one_workgroup(int n, int64_t* sh, In in, Put put) {
    int64_t carry = 0;
    for (int t0 = 0; t0 < n; t0 += NT) {
        const int i = t0 + threadIdx.x;
        const int64_t v = i < n ? (int64_t)in(i) : 0;
        const int64_t before = block_excl_sum<NT>(v, sh);
        if (i < n) put(i, carry + before);
        if (threadIdx.x == NT - 1) sh[0] = before + v;
        __syncthreads();
        carry += sh[0];
        __syncthreads();
    }
    return carry;
}

// ---- rows: raw[p] for p in [0, 3 * w * h): row p / (3 w), R, G, B per pixel, differenced against the pixel to the left
__global__ __launch_bounds__(NT) void tiff_enc_rows_kernel(const maf_tiff_enc_job_t* jobs, int n_files, uint8_t* raw) {
    const int ch = blockIdx.x;
    const maf_tiff_enc_job_t j = jobs[job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; })];
    const int64_t rowlen = 3 * (int64_t)j.w, n = rowlen * j.h;
    const int64_t p0 = (int64_t)(ch - j.chunk0) * CHUNK + 16 * threadIdx.x;
    if (p0 >= n) return;
    int64_t y = p0 / rowlen;
    int c = (int)(p0 - y * rowlen), px = c / 3, k = c - 3 * px;
    const uint8_t* row = static_cast<const uint8_t*>(j.src) + y * j.pitch;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (p0 + i < n) {
            const uint8_t* at = row + 3 * px + 2 - k;                           // R, G, B in the file; B, G, R in the frame
            uint32_t v = at[0];
            if (j.predictor && px > 0) v = (v - at[-3]) & 255u;
            w[i >> 2] |= v << (8 * (i & 3));
            if (++k == 3) { k = 0; ++px; }
            if (++c == rowlen) { c = 0; px = 0; k = 0; row += j.pitch; }
        }
    }
    const u32x4_t v = {w[0], w[1], w[2], w[3]};
    *reinterpret_cast<u32x4_t*>(raw + j.raw_off + p0) = v;                       // the file's region is a multiple of 16 bytes
}

// ---- LZW: one wave per strip.  A dictionary slot is (prefix code 12 | byte 8 | code 12), 0 when empty (a code is at least 258).
__device__ __forceinline__ uint32_t slot_of(uint32_t key) { return (key * 2654435761u) >> 19; }      // 20-bit key -> 13 bits
static_assert(TABLE == 1 << 13, "slot_of");

__global__ __launch_bounds__(64) void tiff_enc_lzw_kernel(const maf_tiff_enc_job_t* jobs, int n_files, const uint8_t* raw, uint16_t* codes,
                                                           maf_tiff_enc_strip_t* strips) {
    __shared__ uint32_t table[TABLE];
    __shared__ __attribute__((aligned(16))) uint8_t in[TILE];
    __shared__ uint16_t cbuf[CODE_CAP];
    __shared__ int sh_pos, sh_codes, sh_clear;
    const int s = blockIdx.x, lane = threadIdx.x;
    const maf_tiff_enc_job_t j = jobs[job_of(n_files, s, [&](int i) { return jobs[i].strip0; })];
    const int k = s - j.strip0;
    const int64_t rowlen = 3 * (int64_t)j.w, full = rowlen * j.rows_per_strip;
    const int n = (int)(rowlen * min(j.rows_per_strip, j.h - k * j.rows_per_strip));      // below MAF_TIFF_ENC_MAX_STRIP
    const uint8_t* src = raw + j.raw_off + (int64_t)k * full;
    uint16_t* dst = codes + j.code_off + (int64_t)k * j.code_slot;
    for (int i = lane; i < TABLE / 4; i += 64) reinterpret_cast<u32x4_t*>(table)[i] = u32x4_t{0u, 0u, 0u, 0u};
    auto fetch = [&](int t0, uint8_t* b) {                                       // the tile at t0: byte lane + 64 i is lane's b[i]
#pragma unroll
        for (int i = 0; i < 16; ++i) b[i] = t0 + lane + 64 * i < n ? src[t0 + lane + 64 * i] : (uint8_t)0;
    };
    auto stage = [&](const uint8_t* b) {
#pragma unroll
        for (int i = 0; i < 16; ++i) in[lane + 64 * i] = b[i];
    };
    uint8_t ahead[16];
    fetch(0, ahead);
    stage(ahead);
    if (lane == 0) { sh_pos = 0; sh_codes = 0; sh_clear = 0; }
    __syncthreads();
    // lane 0's state (tests/tiff_encode_ref.py lzw).  A strip is below 2^23 bytes (MAF_TIFF_ENC_MAX_STRIP), so libtiff's other ratio formula, for
    // input counts above 0x007fffff, is never reached, and (incount << 8) fits 32 bits
    uint32_t ent = 0u, free_ent = FIRST, nbits = 9u, incount = 0u, outcount = 0u, ratio = 0u, checkpoint = CHECK_GAP;
    int total_codes = 0, total_bits = 0;
    bool fresh = true;                                                           // the first pass over a tile
    for (int t0 = 0; t0 < n;) {
        const int tile_n = min(TILE, n - t0);
        if (fresh && t0 + TILE < n) fetch(t0 + TILE, ahead);                     // the next tile is in flight while lane 0 walks
        fresh = false;
        if (lane == 0) {
            int pos = sh_pos, nc = 0, clear = 0;
            auto put = [&](uint32_t code) {
                cbuf[nc++] = (uint16_t)(code | ((nbits - 9u) << 12));
                outcount += nbits;
                total_bits += (int)nbits;
            };
            auto reset = [&]() {
                free_ent = FIRST; ratio = 0u; incount = 0u; outcount = 0u;
                put(CLEAR);                                                      // at the old width
                nbits = 9u;
                clear = 1;
            };
            if (t0 == 0 && pos == 0) {
                put(CLEAR);
                ent = in[0];
                incount = 1u;
                pos = 1;
            }
            while (pos < tile_n && !clear) {
                const uint32_t c = in[pos++];
                ++incount;
                const uint32_t key = (ent << 8) | c;
                uint32_t h = slot_of(key), slot;
                while ((slot = table[h]) != 0u && (slot >> 12) != key) h = (h + 1u) & (TABLE - 1);
                if (slot) { ent = slot & 0xFFFu; continue; }
                put(ent);
                table[h] = (key << 12) | free_ent;
                ent = c;
                ++free_ent;
                if (free_ent == TABLE_FULL) {
                    reset();
                } else if (free_ent > (1u << nbits) - 1u) {
                    ++nbits;
                } else if (incount >= checkpoint) {
                    checkpoint = incount + CHECK_GAP;                            // never reset by reset()
                    const uint32_t rat = (incount << 8) / outcount;
                    if (rat <= ratio) reset(); else ratio = rat;
                }
            }
            if (pos == tile_n && t0 + tile_n == n && !clear) {                   // the strip's end: the last code, then the EOI
                put(ent);
                ++free_ent;
                if (free_ent == TABLE_FULL) { put(CLEAR); nbits = 9u; }
                else if (free_ent > (1u << nbits) - 1u) ++nbits;
                put(EOI);
                pos = tile_n + 1;                                                // done
            }
            sh_pos = pos; sh_codes = nc; sh_clear = clear;
        }
        __syncthreads();
        const int pos = sh_pos, nc = sh_codes, clear = sh_clear;
        for (int i = lane; i < nc; i += 64)
            if (total_codes + i < j.code_slot) dst[total_codes + i] = cbuf[i];      // always (MAF_TIFF_ENC_CODE_BOUND)
        total_codes += nc;
        if (clear)
            for (int i = lane; i < TABLE / 4; i += 64) reinterpret_cast<u32x4_t*>(table)[i] = u32x4_t{0u, 0u, 0u, 0u};
        __syncthreads();
        if (pos > tile_n) break;                                                 // the EOI is out
        if (pos == tile_n && t0 + tile_n < n) {                                  // the next tile
            stage(ahead);
            if (lane == 0) sh_pos = 0;
            t0 += TILE;
            fresh = true;
        }
        // else: a reset in the middle of the tile (or at its end, with the strip's end still to write): walk on from sh_pos
        __syncthreads();
    }
    if (lane == 0) {
        strips[s].n_codes = min(total_codes, j.code_slot);
        strips[s].bits = total_bits;
        strips[s].offset = 0u;
        strips[s].bytes = (uint32_t)((total_bits + 7) >> 3);
    }
}

// bytes of a file behind its strips and the pad byte: BitsPerSample, the two strip arrays (inline for one strip), the IFD
__device__ __forceinline__ int tail_bytes(const maf_tiff_enc_job_t& j) {
    return 6 + (j.n_strips > 1 ? 8 * j.n_strips : 0) + 2 + 12 * (j.predictor ? 11 : 10) + 4;
}

__global__ __launch_bounds__(NT) void tiff_enc_layout_kernel(const maf_tiff_enc_job_t* jobs, maf_tiff_enc_strip_t* strips, int32_t* lengths) {
    __shared__ int64_t sh[NT];
    const maf_tiff_enc_job_t j = jobs[blockIdx.x];
    maf_tiff_enc_strip_t* st = strips + j.strip0;
    const int64_t total = scan_by_one_workgroup(j.n_strips, sh, [&](int i) { return st[i].bytes; }, [&](int i, int64_t before) { st[i].offset = (uint32_t)(8 + before); });
    if (threadIdx.x == 0) {
        const int64_t end = 8 + total;
        lengths[blockIdx.x] = (int32_t)(end + (end & 1) + tail_bytes(j));        // below 2^31 (MAF_TIFF_ENC_MAX_FILE)
    }
}

__global__ __launch_bounds__(NT) void tiff_enc_offsets_kernel(int n_files, const int32_t* lengths, int64_t* offsets) {
    __shared__ int64_t sh[NT];
    scan_by_one_workgroup(n_files, sh, [&](int i) { return lengths[i]; }, [&](int i, int64_t before) { offsets[i] = before; });
}

// ---- pack: the codes MSB first, or-ed into the zeroed output as big-endian 32-bit words
__global__ __launch_bounds__(NT) void tiff_enc_pack_kernel(const maf_tiff_enc_job_t* jobs, int n_files, const uint16_t* codes, const maf_tiff_enc_strip_t* strips,
                                                            const int64_t* offsets, uint8_t* out, int64_t out_bytes) {
    __shared__ int sh[NT];
    __shared__ int tile_bits;
    const int s = blockIdx.x;
    const int f = job_of(n_files, s, [&](int i) { return jobs[i].strip0; });
    const maf_tiff_enc_job_t j = jobs[f];
    const maf_tiff_enc_strip_t st = strips[s];
    const uint16_t* src = codes + j.code_off + (int64_t)(s - j.strip0) * j.code_slot;
    uint32_t* words = reinterpret_cast<uint32_t*>(out);
    const int64_t n_words = out_bytes >> 2;
    const int n_codes = min(st.n_codes, j.code_slot);
    int64_t at = 8 * (offsets[f] + (int64_t)st.offset);
    const int64_t end = at + 8 * (int64_t)st.bytes;                              // the strip's share of the output, in bits
    for (int t0 = 0; t0 < n_codes; t0 += NT * PACK_ITEMS) {                      // a thread owns PACK_ITEMS codes in a row: one scan per tile
        const int i0 = t0 + PACK_ITEMS * threadIdx.x;
        uint32_t val[PACK_ITEMS];
        int nb[PACK_ITEMS], total = 0;
#pragma unroll
        for (int e = 0; e < PACK_ITEMS; ++e) {
            val[e] = 0u; nb[e] = 0;
            if (i0 + e < n_codes) {
                const uint32_t c = src[i0 + e];
                val[e] = c & 0xFFFu;
                nb[e] = 9 + (int)((c >> 12) & 3u);
            }
            total += nb[e];
        }
        const int before = block_excl_sum<NT>(total, sh);
        int64_t bit = at + before;
        int64_t word = bit >> 5;
        int fill = (int)(bit & 31);                                              // bits of `word` in front of this thread's
        uint64_t acc = 0;                                                        // gathered from bit 63 down
        bool shared = true;                                                      // the first word may hold the end of the thread before
        auto flush = [&](uint32_t v, bool whole) {
            if (word < n_words) {
                const uint32_t be = __builtin_bswap32(v);
                if (whole && !shared) words[word] = be; else if (be) atomicOr(words + word, be);
            }
        };
#pragma unroll
        for (int e = 0; e < PACK_ITEMS; ++e) {
            if (!nb[e] || bit + nb[e] > end) continue;                           // never: st.bits is the sum of the widths
            acc |= (uint64_t)val[e] << (64 - fill - nb[e]);
            fill += nb[e];
            bit += nb[e];
            if (fill >= 32) {
                flush((uint32_t)(acc >> 32), true);
                shared = false;
                acc <<= 32;
                fill -= 32;
                ++word;
            }
        }
        if (fill > 0) flush((uint32_t)(acc >> 32), false);                       // shared with the thread behind
        if (threadIdx.x == NT - 1) tile_bits = before + total;
        __syncthreads();
        at += tile_bits;
        __syncthreads();
    }
}

// ---- the file around the strips (tests/tiff_encode_ref.py assemble)
__global__ __launch_bounds__(NT) void tiff_enc_frame_kernel(const maf_tiff_enc_job_t* jobs, const maf_tiff_enc_strip_t* strips, const int32_t* lengths,
                                                             const int64_t* offsets, uint8_t* out, int64_t out_bytes) {
    const int f = blockIdx.x;
    const maf_tiff_enc_job_t j = jobs[f];
    const maf_tiff_enc_strip_t* st = strips + j.strip0;
    const int64_t o = offsets[f];
    const int n = j.n_strips;
    const uint32_t bits_at = (uint32_t)(lengths[f] - tail_bytes(j));             // even: behind the strips and the pad byte
    auto put16 = [&](int64_t at, uint32_t v) {
        for (int i = 0; i < 2; ++i)
            if (o + at + i < out_bytes) out[o + at + i] = (uint8_t)(v >> (8 * i));
    };
    auto put32 = [&](int64_t at, uint32_t v) {
        for (int i = 0; i < 4; ++i)
            if (o + at + i < out_bytes) out[o + at + i] = (uint8_t)(v >> (8 * i));
    };
    if (n > 1)
        for (int i = threadIdx.x; i < n; i += NT) {
            put32((int64_t)bits_at + 6 + 4 * (int64_t)i, st[i].offset);
            put32((int64_t)bits_at + 6 + 4 * (int64_t)(n + i), st[i].bytes);
        }
    if (threadIdx.x != 0) return;
    const uint32_t ifd_at = bits_at + 6u + (n > 1 ? 8u * (uint32_t)n : 0u);
    put32(0, 0x002A4949u);                                                       // II*\0
    put32(4, ifd_at);
    for (int i = 0; i < 3; ++i) put16((int64_t)bits_at + 2 * i, 8u);
    int64_t at = ifd_at;
    auto entry = [&](uint32_t tag, uint32_t type, uint32_t count, uint32_t value) {
        put16(at, tag); put16(at + 2, type); put32(at + 4, count); put32(at + 8, value);
        at += 12;
    };
    constexpr uint32_t SHORT = 3u, LONG = 4u;
    put16(at, j.predictor ? 11u : 10u);
    at += 2;
    entry(256u, SHORT, 1u, (uint32_t)j.w);
    entry(257u, SHORT, 1u, (uint32_t)j.h);
    entry(258u, SHORT, 3u, bits_at);
    entry(259u, SHORT, 1u, 5u);                                                  // LZW
    entry(262u, SHORT, 1u, 2u);                                                  // RGB
    entry(273u, LONG, (uint32_t)n, n > 1 ? bits_at + 6u : st[0].offset);
    entry(277u, SHORT, 1u, 3u);
    entry(278u, SHORT, 1u, (uint32_t)j.rows_per_strip);
    entry(279u, LONG, (uint32_t)n, n > 1 ? bits_at + 6u + 4u * (uint32_t)n : st[0].bytes);
    entry(284u, SHORT, 1u, 1u);
    if (j.predictor) entry(317u, SHORT, 1u, 2u);
    put32(at, 0u);
}

}  // namespace

extern "C" int maf_tiff_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "tiff_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_tiff_enc_header_t); out[1] = (int32_t)sizeof(maf_tiff_enc_job_t); out[2] = (int32_t)sizeof(maf_tiff_enc_strip_t);
    return 0;
}

extern "C" int maf_tiff_encode(const void* blob_host, const void* blob_dev, uint8_t* raw, uint16_t* codes, void* strips, uint8_t* out, int32_t* lengths,
                               int64_t* offsets, maf_tiff_enc_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && raw && codes && strips && out && lengths && offsets, "tiff_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, raw}) && maf_aligned({offsets}, 8) && maf_aligned({out, strips, lengths}, 4) && maf_aligned({codes}, 2),
                "tiff_encode: blob and raw must be 16-byte aligned, offsets 8-byte, out, strips and lengths 4-byte, codes 2-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_tiff_enc_header_t hd = maf_blob_header<maf_tiff_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files), "tiff_encode: 1 to 65535 files per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "tiff_encode: blob size out of range");
    MAF_REQUIRE(hd.n_strips > 0 && hd.n_strips < (1 << 30) && hd.n_chunks > 0 && hd.n_chunks < (1 << 30), "tiff_encode: strip or chunk count out of range");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(maf_tiff_enc_job_t), T), "tiff_encode: the job table lies outside the blob");
    const maf_tiff_enc_job_t* jobs = reinterpret_cast<const maf_tiff_enc_job_t*>(hb + hd.jobs_off);
    int64_t strip = 0, chunk = 0, at_raw = 0, at_code = 0, need = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const maf_tiff_enc_job_t& j = jobs[i];
        MAF_REQUIRE(j.src, "tiff_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= 65535 && j.h <= 65535, "tiff_encode: width and height are 1 to 65535");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "tiff_encode: a row pitch below 3 * width");
        MAF_REQUIRE(j.predictor == 0 || j.predictor == 1, "tiff_encode: predictor is 0 or 1");
        MAF_REQUIRE(j.rows_per_strip >= 1 && j.rows_per_strip <= j.h, "tiff_encode: rows_per_strip outside 1..h");
        const int64_t full = 3 * (int64_t)j.w * j.rows_per_strip, n = 3 * (int64_t)j.w * j.h;
        MAF_REQUIRE(full < MAF_TIFF_ENC_MAX_STRIP, "tiff_encode: a strip of 8 MiB or more");
        const int64_t ns = (j.h + j.rows_per_strip - 1) / j.rows_per_strip;
        const int64_t last = n - (ns - 1) * full;
        const int64_t bound = 8 + (ns - 1) * MAF_TIFF_ENC_BYTE_BOUND(full) + MAF_TIFF_ENC_BYTE_BOUND(last) + 1 + 6 + (ns > 1 ? 8 * ns : 0) + 2 + 12 * (j.predictor ? 11 : 10) + 4;
        MAF_REQUIRE(bound < MAF_TIFF_ENC_MAX_FILE, "tiff_encode: a file whose worst case is 2 GiB or more");
        MAF_REQUIRE(j.n_strips == ns && j.strip0 == strip, "tiff_encode: the files' strips must follow each other");
        MAF_REQUIRE(j.n_chunks == (n + CHUNK - 1) / CHUNK && j.chunk0 == chunk, "tiff_encode: the files' chunks must follow each other");
        MAF_REQUIRE(j.code_slot == MAF_TIFF_ENC_CODE_BOUND(full), "tiff_encode: a code slot that is not the bound of a full strip");
        MAF_REQUIRE(j.raw_off == at_raw && j.code_off == at_code, "tiff_encode: the files' regions must follow each other without gaps");
        strip += ns;
        chunk += j.n_chunks;
        at_raw += (n + 15) / 16 * 16;
        at_code += ns * (int64_t)j.code_slot;
        need += bound;
        MAF_REQUIRE(strip < (1 << 30) && chunk < (1 << 30), "tiff_encode: strip or chunk count out of range");
    }
    MAF_REQUIRE(strip == hd.n_strips && chunk == hd.n_chunks, "tiff_encode: the header's strip or chunk count differs from the jobs' sum");
    MAF_REQUIRE(hd.raw_bytes >= at_raw && hd.code_elems >= at_code && hd.out_bytes >= need && (hd.out_bytes & 3) == 0,
                "tiff_encode: a device buffer is smaller than the worst case, or out is not a multiple of 4 bytes");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_tiff_enc_job_t* d_jobs = reinterpret_cast<const maf_tiff_enc_job_t*>(db + hd.jobs_off);
    maf_tiff_enc_strip_t* d_strips = static_cast<maf_tiff_enc_strip_t*>(strips);
    const int rc = maf_check_hip(hipMemsetAsync(out, 0, (size_t)hd.out_bytes, s), "tiff_encode memset out");
    if (rc) return rc;
    hipLaunchKernelGGL(tiff_enc_rows_kernel, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, raw);
    MAF_LAUNCH_CHECK("tiff_enc_rows");
    hipLaunchKernelGGL(tiff_enc_lzw_kernel, dim3(hd.n_strips), dim3(64), 0, s, d_jobs, hd.n_files, raw, codes, d_strips);
    MAF_LAUNCH_CHECK("tiff_enc_lzw");
    hipLaunchKernelGGL(tiff_enc_layout_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, d_strips, lengths);
    MAF_LAUNCH_CHECK("tiff_enc_layout");
    hipLaunchKernelGGL(tiff_enc_offsets_kernel, dim3(1), dim3(NT), 0, s, hd.n_files, lengths, offsets);
    MAF_LAUNCH_CHECK("tiff_enc_offsets");
    hipLaunchKernelGGL(tiff_enc_pack_kernel, dim3(hd.n_strips), dim3(NT), 0, s, d_jobs, hd.n_files, codes, d_strips, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("tiff_enc_pack");
    hipLaunchKernelGGL(tiff_enc_frame_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, d_strips, lengths, offsets, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("tiff_enc_frame");
    return 0;
}
