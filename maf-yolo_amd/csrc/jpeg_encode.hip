// Baseline JPEG encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any row pitch), the files
// libjpeg writes with its defaults out (jpeg_set_quality + force_baseline, JDCT_ISLOW, 4:2:0 or 4:4:4, standard Huffman tables, JFIF header),
// bit for bit.  Replaces save_one_box and the final cv2.imwrite of Inferer.infer (yolov6/core/inferer.py).  The rules are restated in
// tests/jpeg_encode_ref.py (its docstring lists every one with the libjpeg file it comes from); the host side (tables, headers, buffer
// sizes) is maf-yolo_amd/jpeg_encode.py.
//
// Nine kernels, one launch each for the whole batch (include/mafyolo_hip.h describes the blob and the buffers), plus one memset:
//   jpeg_enc_transform_kernel  jccolor.c + jcsample.c + jfdctint.c + jcdctmgr.c.  One thread per 8 x 8 block, blocks in coded order: the pixels
//                              come straight from the frame (edge padding = clamped indices; a 4:2:0 chroma sample is the biased mean of its 2 x 2
//                              pixels, the rows clamped AFTER downsampling as jcprepct.c pads), the two FDCT passes run in registers, the
//                              quantised coefficients leave as 8 x 16-byte stores in zigzag order.  Dummy blocks are stored as zeros.
//   jpeg_enc_count_kernel      jchuff.c, sizes only.  The DC predictor is a lookup: the nearest real block of the same component coded before
//                              (at most 4 + 4 candidates in 4:2:0), not a chain.  A dummy block receives that DC (jccoefct.c) and costs the DC code
//                              of category 0 + EOB.  Also the sum of every 256 counts.
//   jpeg_enc_sums_kernel       one workgroup: exclusive scan of those sums (64-bit, tiles of 256 with a carry).
//   jpeg_enc_offsets_kernel    exclusive scan of the counts inside each 256 + its sum's offset -> the bit offset of every block in the batch.
//   jpeg_enc_pack_kernel       jchuff.c, the bits.  A thread gathers its block's codes in a 64-bit window aligned to the 32-bit words of the
//                              file's packed region and stores whole words; the first and the last word it touches may be shared with the
//                              neighbouring blocks and are combined with atomicOr (the region is zeroed by the memset in front: a buffer
//                              the caching allocator hands back holds an earlier call's bits).  The file's last block adds the 1-bits fill.
//   jpeg_enc_ffcount_kernel    0xFF bytes per MAF_JPEG_ENC_CHUNK of each file's packed bytes (16 bytes per thread).
//   jpeg_enc_ffscan_kernel     one workgroup per file: exclusive scan of its chunks' counts; the file's length.
//   jpeg_enc_lenscan_kernel    one workgroup: exclusive scan of the lengths -> where each file starts in the output.
//   jpeg_enc_stuff_kernel      header, scan with 0x00 behind every 0xFF, EOI.
// Every index that depends on pixel content (bit offsets, 0xFF counts) is bounded by construction (MAF_JPEG_ENC_BLOCK_BITS per block: the
// sizes are clamped to what the standard tables code) and compared with the region's size before a store all the same.
#include "maf_common.h"
#include "jpeg_bits.h"
#include "block_scan.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MAF_JPEG_ENC_CHUNK;
static_assert(CHUNK == 16 * NT, "a thread of the stuffing kernels owns 16 bytes of a chunk");
static_assert(MAF_JPEG_ENC_BLOCK_BYTES * 8 >= MAF_JPEG_ENC_BLOCK_BITS && MAF_JPEG_ENC_BLOCK_BITS == 22 + 63 * 26, "worst case of a block");

// the last job whose first block (FIELD = block0) or first chunk (chunk0) is at most i
template <typename F>
__device__ __forceinline__ int job_of(int n, int i, F first) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first(mid) <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

struct BlockPos { int comp, bx, by; bool real; };

// block `k` of MCU `m` of a file: its component, its place in the component's block grid, and whether the image reaches it (jccoefct.c)
__device__ __forceinline__ BlockPos block_pos(const maf_jpeg_enc_job_t& j, int m, int k) {
    const int my = m / j.mcux, mx = m - my * j.mcux, ny = j.hs * j.hs;
    BlockPos p;
    if (k < ny) {
        const int v = j.hs == 2 ? k >> 1 : 0, h = j.hs == 2 ? k & 1 : 0;
        p.comp = 0; p.bx = mx * j.hs + h; p.by = my * j.hs + v;
        p.real = p.bx < (j.w + 7) / 8 && p.by < (j.h + 7) / 8;
    } else {
        p.comp = 1 + k - ny; p.bx = mx; p.by = my; p.real = true;       // ceil(ceil(w / hs) / 8) = mcux: chroma has no dummy blocks
    }
    return p;
}

// the block whose DC predicts block (m, k): the nearest real block of the same component coded before it (local index), -1 at the start of the scan
__device__ __forceinline__ int prev_real(const maf_jpeg_enc_job_t& j, int m, int k) {
    const int ny = j.hs * j.hs, bpm = ny + 2;
    if (k >= ny) return m > 0 ? (m - 1) * bpm + k : -1;
    for (int kk = k - 1; kk >= 0; --kk)
        if (block_pos(j, m, kk).real) return m * bpm + kk;
    if (m == 0) return -1;
    for (int kk = ny - 1; kk > 0; --kk)
        if (block_pos(j, m - 1, kk).real) return (m - 1) * bpm + kk;
    return (m - 1) * bpm;                                                // block 0 of an MCU is always real
}

// ---- jfdctint.c jpeg_fdct_islow (constants: jpeg_bits.h)

template <int N>
__device__ __forceinline__ int descale(int x) { return (x + (1 << (N - 1))) >> N; }

template <bool FIRST>
__device__ __forceinline__ void fdct_1d(const int d[8], int o[8]) {
    const int tmp0 = d[0] + d[7], tmp7 = d[0] - d[7], tmp1 = d[1] + d[6], tmp6 = d[1] - d[6];
    const int tmp2 = d[2] + d[5], tmp5 = d[2] - d[5], tmp3 = d[3] + d[4], tmp4 = d[3] - d[4];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int N = FIRST ? CONST_BITS - PASS1_BITS : CONST_BITS + PASS1_BITS;
    if (FIRST) {
        o[0] = (tmp10 + tmp11) * (1 << PASS1_BITS); o[4] = (tmp10 - tmp11) * (1 << PASS1_BITS);
    } else {
        o[0] = descale<PASS1_BITS>(tmp10 + tmp11); o[4] = descale<PASS1_BITS>(tmp10 - tmp11);
    }
    int z1 = (tmp12 + tmp13) * FIX_0_541196100;
    o[2] = descale<N>(z1 + tmp13 * FIX_0_765366865);
    o[6] = descale<N>(z1 + tmp12 * (-FIX_1_847759065));
    z1 = tmp4 + tmp7;
    int z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    const int t4 = tmp4 * FIX_0_298631336, t5 = tmp5 * FIX_2_053119869, t6 = tmp6 * FIX_3_072711026, t7 = tmp7 * FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    o[7] = descale<N>(t4 + z1 + z3); o[5] = descale<N>(t5 + z2 + z4);
    o[3] = descale<N>(t6 + z2 + z3); o[1] = descale<N>(t7 + z1 + z4);
}

// jccolor.c rgb_ycc_convert: the sample of component `comp` of a BGR pixel
struct ColorRow { int kr, kg, kb, add; };
__device__ __forceinline__ ColorRow color_row(int comp) {
    if (comp == 0) return {19595, 38470, 7471, 32768};
    if (comp == 1) return {-11059, -21709, 32768, (128 << 16) + 32767};
    return {32768, -27439, -5329, (128 << 16) + 32767};
}
__device__ __forceinline__ int sample_at(const uint8_t* px, const ColorRow& k) { return (k.kr * px[2] + k.kg * px[1] + k.kb * px[0] + k.add) >> 16; }

__global__ __launch_bounds__(NT) void jpeg_enc_transform_kernel(const maf_jpeg_enc_job_t* jobs, int n_files, int n_blocks, const uint16_t* quant, int16_t* coef) {
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= n_blocks) return;
    const maf_jpeg_enc_job_t j = jobs[job_of(n_files, b, [&](int i) { return jobs[i].block0; })];
    const int bpm = j.hs * j.hs + 2, local = b - j.block0, m = local / bpm;
    const BlockPos p = block_pos(j, m, local - m * bpm);
    u32x4_t* dst = reinterpret_cast<u32x4_t*>(coef + 64 * (int64_t)b);
    if (!p.real) {
        const u32x4_t zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int r = 0; r < 8; ++r) dst[r] = zero;
        return;
    }
    const uint8_t* src = static_cast<const uint8_t*>(j.src);
    const ColorRow k = color_row(p.comp);
    int ws[64];
    if (p.comp == 0 || j.hs == 1) {
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint8_t* row = src + (int64_t)min(8 * p.by + r, j.h - 1) * j.pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) ws[8 * r + c] = sample_at(row + 3 * min(8 * p.bx + c, j.w - 1), k) - 128;
        }
    } else {                                                     // h2v2_downsample: columns clamped in the input, rows in the downsampled plane
        const int dh = (j.h + 1) >> 1;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = min(8 * p.by + r, dh - 1);
            const uint8_t* r0 = src + (int64_t)(2 * y) * j.pitch;
            const uint8_t* r1 = src + (int64_t)min(2 * y + 1, j.h - 1) * j.pitch;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const int x = 8 * p.bx + c, x0 = 3 * min(2 * x, j.w - 1), x1 = 3 * min(2 * x + 1, j.w - 1);
                ws[8 * r + c] = ((sample_at(r0 + x0, k) + sample_at(r0 + x1, k) + sample_at(r1 + x0, k) + sample_at(r1 + x1, k) + 1 + (c & 1)) >> 2) - 128;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 8; ++r) {                                // pass 1: rows
        int o[8];
        fdct_1d<true>(&ws[8 * r], o);
#pragma unroll
        for (int c = 0; c < 8; ++c) ws[8 * r + c] = o[c];
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) {                                // pass 2: columns
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[8 * r + c];
        fdct_1d<false>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[8 * r + c] = o[r];
    }
    const uint16_t* q = quant + (p.comp ? 64 : 0);
    uint32_t out[32];
    maf_static_for<64>([&](auto zi) {                            // jcdctmgr.c: divisor q * 8, |c| rounded half up, sign restored; zigzag order
        constexpr int z = decltype(zi)::value;
        const int c = ws[ZZ[z]];
        const uint32_t div = (uint32_t)q[ZZ[z]] << 3;
        const int v = (int)(((uint32_t)abs(c) + (div >> 1)) / div);
        const uint32_t h = (uint32_t)(c < 0 ? -v : v) & 0xFFFFu;
        if (z & 1) out[z >> 1] |= h << 16; else out[z >> 1] = h;
    });
#pragma unroll
    for (int r = 0; r < 8; ++r) {
        const u32x4_t v = {out[4 * r], out[4 * r + 1], out[4 * r + 2], out[4 * r + 3]};
        dst[r] = v;
    }
}

// ---- jchuff.c encode_one_block over the stored block: emit(code, length) for every code with its value bits appended
__device__ __forceinline__ int bit_size(int v, int most) { return min(32 - __clz(abs(v)), most); }

template <typename Emit>
__device__ __forceinline__ void encode_block(const int16_t* blk, int pred, const uint32_t* dct, const uint32_t* act, Emit&& emit) {
    const u32x4_t* in = reinterpret_cast<const u32x4_t*>(blk);
    int run = 0;
    for (int v = 0; v < 8; ++v) {
        const u32x4_t a = in[v];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int c = (int)(int16_t)((i & 1) ? a[i >> 1] >> 16 : a[i >> 1] & 0xFFFFu);
            if (i == 0 && v == 0) {
                const int d = c - pred, s = bit_size(d, 11);
                const uint32_t e = dct[s];
                emit(((e & 0xFFFFu) << s) | ((uint32_t)(d < 0 ? d - 1 : d) & ((1u << s) - 1u)), (int)(e >> 16) + s);
            } else if (c == 0) {
                ++run;
            } else {
                for (; run > 15; run -= 16) emit(act[0xF0] & 0xFFFFu, (int)(act[0xF0] >> 16));
                const int s = bit_size(c, 10);
                const uint32_t e = act[(run << 4) | s];
                emit(((e & 0xFFFFu) << s) | ((uint32_t)(c < 0 ? c - 1 : c) & ((1u << s) - 1u)), (int)(e >> 16) + s);
                run = 0;
            }
        }
    }
    if (run > 0) emit(act[0] & 0xFFFFu, (int)(act[0] >> 16));
}

__device__ __forceinline__ void load_codes(const uint32_t* huff, uint32_t* tab) {
    for (int i = threadIdx.x; i < 1024; i += NT) tab[i] = huff[i];
    __syncthreads();
}

__global__ __launch_bounds__(NT) void jpeg_enc_count_kernel(const maf_jpeg_enc_job_t* jobs, int n_files, int n_blocks, const uint32_t* huff, int16_t* coef,
                                                             int32_t* bits, int64_t* sums) {
    __shared__ uint32_t tab[1024];
    __shared__ int sh[NT];
    load_codes(huff, tab);
    const int b = blockIdx.x * NT + threadIdx.x;
    int nb = 0;
    if (b < n_blocks) {
        const maf_jpeg_enc_job_t j = jobs[job_of(n_files, b, [&](int i) { return jobs[i].block0; })];
        const int bpm = j.hs * j.hs + 2, local = b - j.block0, m = local / bpm, k = local - m * bpm;
        const BlockPos p = block_pos(j, m, k);
        const uint32_t* dct = tab + (p.comp ? 256 : 0);
        const uint32_t* act = tab + 512 + (p.comp ? 256 : 0);
        const int pr = prev_real(j, m, k);
        const int pred = pr < 0 ? 0 : coef[64 * (int64_t)(j.block0 + pr)];       // a REAL block's DC: no thread of this launch writes it
        if (!p.real) {
            coef[64 * (int64_t)b] = (int16_t)pred;
            nb = (int)(dct[0] >> 16) + (int)(act[0] >> 16);
        } else {
            encode_block(coef + 64 * (int64_t)b, pred, dct, act, [&](uint32_t, int len) { nb += len; });
        }
        bits[b] = nb;
    }
    const int before = block_excl_sum<NT>(nb, sh);
    if (threadIdx.x == NT - 1) sums[blockIdx.x] = before + nb;
}

// exclusive scan of in[0 .. n) into out[0 .. n) by ONE workgroup; returns the total
template <typename TI, typename TO>
__device__ __forceinline__ int64_t scan_by_one_workgroup(const TI* in, TO* out, int n, int64_t* sh) {
    int64_t carry = 0;
    for (int t0 = 0; t0 < n; t0 += NT) {
        const int i = t0 + threadIdx.x;
        const int64_t v = i < n ? (int64_t)in[i] : 0;
        const int64_t before = block_excl_sum<NT>(v, sh);
        if (i < n) out[i] = (TO)(carry + before);
        if (threadIdx.x == NT - 1) sh[0] = before + v;           // block_excl_sum has left sh free
        __syncthreads();
        carry += sh[0];
        __syncthreads();
    }
    return carry;
}

__global__ __launch_bounds__(NT) void jpeg_enc_sums_kernel(int64_t* sums, int n_sums) {
    __shared__ int64_t sh[NT];
    scan_by_one_workgroup(sums, sums + n_sums, n_sums, sh);
}

__global__ __launch_bounds__(NT) void jpeg_enc_offsets_kernel(const int32_t* bits, const int64_t* sums, int n_sums, int n_blocks, int64_t* bitoff) {
    __shared__ int sh[NT];
    const int b = blockIdx.x * NT + threadIdx.x;
    const int nb = b < n_blocks ? bits[b] : 0;
    const int before = block_excl_sum<NT>(nb, sh);
    if (b >= n_blocks) return;
    const int64_t at = sums[n_sums + blockIdx.x] + before;
    bitoff[b] = at;
    if (b == n_blocks - 1) bitoff[n_blocks] = at + nb;
}

__global__ __launch_bounds__(NT) void jpeg_enc_pack_kernel(const maf_jpeg_enc_job_t* jobs, int n_files, int n_blocks, const uint32_t* huff, const int16_t* coef,
                                                            const int64_t* bitoff, uint32_t* packed) {
    __shared__ uint32_t tab[1024];
    load_codes(huff, tab);
    const int b = blockIdx.x * NT + threadIdx.x;
    if (b >= n_blocks) return;
    const maf_jpeg_enc_job_t j = jobs[job_of(n_files, b, [&](int i) { return jobs[i].block0; })];
    const int bpm = j.hs * j.hs + 2, local = b - j.block0, m = local / bpm, k = local - m * bpm;
    const BlockPos p = block_pos(j, m, k);
    const uint32_t* dct = tab + (p.comp ? 256 : 0);
    const uint32_t* act = tab + 512 + (p.comp ? 256 : 0);
    const int64_t rel = bitoff[b] - bitoff[j.block0];            // < 2^31: a file holds at most MAF_JPEG_ENC_MAX_BLOCKS blocks
    uint32_t* base = packed + (int64_t)j.chunk0 * (CHUNK / 4);
    const int64_t words = (int64_t)j.n_chunks * (CHUNK / 4);
    int64_t word = rel >> 5;
    int fill = (int)(rel & 31);
    uint64_t acc = 0;                                            // the bits gathered for `word`, most significant first, `fill` of them (the first ones another block's)
    bool shared = true;                                          // the first word may hold the end of the block before
    auto put = [&](uint32_t code, int len) {                     // len <= 26, fill <= 31
        acc |= (uint64_t)code << (64 - fill - len);
        fill += len;
        if (fill >= 32) {
            const uint32_t w = __builtin_bswap32((uint32_t)(acc >> 32));     // byte 0 of the stream in the word's lowest address
            if (word < words) {
                if (shared) atomicOr(base + word, w); else base[word] = w;
            }
            shared = false;
            acc <<= 32;
            fill -= 32;
            ++word;
        }
    };
    if (!p.real) {
        put(dct[0] & 0xFFFFu, (int)(dct[0] >> 16));
        put(act[0] & 0xFFFFu, (int)(act[0] >> 16));
    } else {
        const int pr = prev_real(j, m, k);
        encode_block(coef + 64 * (int64_t)b, pr < 0 ? 0 : coef[64 * (int64_t)(j.block0 + pr)], dct, act, put);
    }
    if (local == j.n_blocks - 1) {                               // jchuff.c flush_bits: the partial byte is filled with 1-bits
        const int pad = (8 - (fill & 7)) & 7;
        if (pad) put((1u << pad) - 1u, pad);
    }
    if (fill > 0 && word < words) atomicOr(base + word, __builtin_bswap32((uint32_t)(acc >> 32)));
}

// bytes of a file's entropy-coded segment before stuffing
__device__ __forceinline__ int64_t packed_bytes(const maf_jpeg_enc_job_t& j, const int64_t* bitoff) {
    return (bitoff[j.block0 + j.n_blocks] - bitoff[j.block0] + 7) >> 3;
}

__device__ __forceinline__ int count_ff(const u32x4_t& v, int valid) {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) n += (i < valid && ((v[i >> 2] >> (8 * (i & 3))) & 0xFFu) == 0xFFu) ? 1 : 0;
    return n;
}

__global__ __launch_bounds__(NT) void jpeg_enc_ffcount_kernel(const maf_jpeg_enc_job_t* jobs, int n_files, const int64_t* bitoff, const uint8_t* packed, int32_t* ffcount) {
    __shared__ int sh[NT];
    const int ch = blockIdx.x;
    const maf_jpeg_enc_job_t j = jobs[job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; })];
    const int64_t nbytes = packed_bytes(j, bitoff), start = (int64_t)(ch - j.chunk0) * CHUNK + 16 * threadIdx.x;
    int n = 0;
    if (start < nbytes) n = count_ff(*reinterpret_cast<const u32x4_t*>(packed + (int64_t)j.chunk0 * CHUNK + start), (int)min(nbytes - start, (int64_t)16));
    const int before = block_excl_sum<NT>(n, sh);
    if (threadIdx.x == NT - 1) ffcount[ch] = before + n;
}

__global__ __launch_bounds__(NT) void jpeg_enc_ffscan_kernel(const maf_jpeg_enc_job_t* jobs, const int64_t* bitoff, int32_t* ffcount, int32_t* lengths) {
    __shared__ int64_t sh[NT];
    const maf_jpeg_enc_job_t j = jobs[blockIdx.x];
    const int64_t nbytes = packed_bytes(j, bitoff);
    const int used = (int)min((nbytes + CHUNK - 1) / CHUNK, (int64_t)j.n_chunks);
    const int64_t ff = scan_by_one_workgroup(ffcount + j.chunk0, ffcount + j.chunk0, used, sh);
    if (threadIdx.x == 0) lengths[blockIdx.x] = (int32_t)(j.head_len + nbytes + ff + 2);
}

__global__ __launch_bounds__(NT) void jpeg_enc_lenscan_kernel(const int32_t* lengths, int64_t* offsets, int n_files) {
    __shared__ int64_t sh[NT];
    scan_by_one_workgroup(lengths, offsets, n_files, sh);
}

__global__ __launch_bounds__(NT) void jpeg_enc_stuff_kernel(const maf_jpeg_enc_job_t* jobs, int n_files, const int64_t* bitoff, const uint8_t* packed, const int32_t* ffcount,
                                                             const int64_t* offsets, const uint8_t* heads, uint8_t* out, int64_t out_bytes) {
    __shared__ int sh[NT];
    const int ch = blockIdx.x;
    const int f = job_of(n_files, ch, [&](int i) { return jobs[i].chunk0; });
    const maf_jpeg_enc_job_t j = jobs[f];
    const int64_t nbytes = packed_bytes(j, bitoff), first = (int64_t)(ch - j.chunk0) * CHUNK;
    if (first >= nbytes) return;                                 // the whole workgroup: a chunk of the worst case the file did not need
    const int64_t at = offsets[f];
    if (ch == j.chunk0)
        for (int i = threadIdx.x; i < j.head_len; i += NT)
            if (at + i < out_bytes) out[at + i] = heads[j.head_off + i];
    const int64_t start = first + 16 * threadIdx.x;
    const int valid = start < nbytes ? (int)min(nbytes - start, (int64_t)16) : 0;
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (valid) v = *reinterpret_cast<const u32x4_t*>(packed + (int64_t)j.chunk0 * CHUNK + start);
    const int before = block_excl_sum<NT>(count_ff(v, valid), sh) + ffcount[ch];
    int64_t o = at + j.head_len + start + before;
    auto store = [&](uint32_t byte) {
        if (o < out_bytes) out[o] = (uint8_t)byte;
        ++o;
    };
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i < valid) {
            const uint32_t byte = (v[i >> 2] >> (8 * (i & 3))) & 0xFFu;
            store(byte);
            if (byte == 0xFFu) store(0u);
        }
    }
    if (valid && start + valid == nbytes) {                      // EOI
        store(0xFFu);
        store(0xD9u);
    }
}

}  // namespace

extern "C" int maf_jpeg_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "jpeg_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_jpeg_enc_header_t); out[1] = (int32_t)sizeof(maf_jpeg_enc_job_t);
    return 0;
}

extern "C" int maf_jpeg_encode(const void* blob_host, const void* blob_dev, int16_t* coef, int32_t* bits, int64_t* bitoff, int64_t* sums, uint8_t* packed,
                               int32_t* ffcount, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && coef && bits && bitoff && sums && packed && ffcount && out && lengths && offsets, "jpeg_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, coef, packed}) && maf_aligned({bitoff, sums, offsets}, 8),
                "jpeg_encode: blob, coef and packed must be 16-byte aligned, the 64-bit buffers 8-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_jpeg_enc_header_t hd = maf_blob_header<maf_jpeg_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files), "jpeg_encode: 1 to 65535 files per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "jpeg_encode: blob size out of range");
    MAF_REQUIRE(hd.n_blocks > 0 && hd.n_blocks < (1 << 30) && hd.n_chunks > 0 && hd.n_chunks < (1 << 30), "jpeg_encode: block or chunk count out of range");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(maf_jpeg_enc_job_t), T) && in_blob(hd.huff_off, 4 * 256 * 4, T) &&
                in_blob(hd.quant_off, 2 * 64 * 2, T) && in_blob(hd.heads_off, hd.heads_bytes, T), "jpeg_encode: a blob section lies outside the blob");
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(hb + hd.huff_off);
    for (int i = 0; i < 1024; ++i)
        MAF_REQUIRE((codes[i] >> 16) <= 16 && (codes[i] & 0xFFFFu) < (1u << (codes[i] >> 16)), "jpeg_encode: a Huffman code longer than 16 bits or wider than its length");
    for (int t = 0; t < 2; ++t) {                                // what the kernels can emit: DC categories 0..11; EOB, ZRL and every run with sizes 1..10
        for (int s = 0; s < 12; ++s) MAF_REQUIRE((codes[256 * t + s] >> 16) > 0, "jpeg_encode: a DC category the encoder can emit has no code");
        for (int rs = 0; rs < 256; ++rs)
            MAF_REQUIRE(((rs & 15) == 0 ? rs != 0 && rs != 0xF0 : (rs & 15) > 10) || (codes[512 + 256 * t + rs] >> 16) > 0,
                        "jpeg_encode: an AC symbol the encoder can emit has no code");
    }
    const uint16_t* qv = reinterpret_cast<const uint16_t*>(hb + hd.quant_off);
    for (int i = 0; i < 128; ++i) MAF_REQUIRE(qv[i] >= 1 && qv[i] <= 255, "jpeg_encode: a quantisation value outside 1..255");
    const maf_jpeg_enc_job_t* jobs = reinterpret_cast<const maf_jpeg_enc_job_t*>(hb + hd.jobs_off);
    int64_t block = 0, chunk = 0, need = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const maf_jpeg_enc_job_t& j = jobs[i];
        MAF_REQUIRE(j.src, "jpeg_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= 65535 && j.h <= 65535, "jpeg_encode: width and height are 1 to 65535");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "jpeg_encode: a row pitch below 3 * width");
        MAF_REQUIRE(j.hs == 1 || j.hs == 2, "jpeg_encode: sampling is 4:2:0 (2) or 4:4:4 (1)");
        MAF_REQUIRE(j.mcux == (j.w + 8 * j.hs - 1) / (8 * j.hs) && j.mcuy == (j.h + 8 * j.hs - 1) / (8 * j.hs), "jpeg_encode: MCU counts do not match the size");
        const int64_t nb = (int64_t)j.mcux * j.mcuy * (j.hs * j.hs + 2);
        MAF_REQUIRE(nb <= MAF_JPEG_ENC_MAX_BLOCKS, "jpeg_encode: more than MAF_JPEG_ENC_MAX_BLOCKS blocks in one file");
        MAF_REQUIRE(j.n_blocks == nb && j.block0 == block, "jpeg_encode: the files' blocks must follow each other without gaps");
        MAF_REQUIRE(j.n_chunks == (nb * MAF_JPEG_ENC_BLOCK_BYTES + CHUNK - 1) / CHUNK && j.chunk0 == chunk, "jpeg_encode: the files' chunks must follow each other, sized by the worst case");
        MAF_REQUIRE(j.head_len > 0 && j.head_off >= 0 && (int64_t)j.head_off + j.head_len <= hd.heads_bytes, "jpeg_encode: a file's header lies outside the section");
        block += nb;
        chunk += j.n_chunks;
        need += j.head_len + 2 + 2 * MAF_JPEG_ENC_BLOCK_BYTES * nb;
    }
    MAF_REQUIRE(block == hd.n_blocks && chunk == hd.n_chunks, "jpeg_encode: the header's block or chunk count differs from the jobs' sum");
    MAF_REQUIRE(hd.out_bytes >= need, "jpeg_encode: the output buffer is smaller than the worst case");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_jpeg_enc_job_t* d_jobs = reinterpret_cast<const maf_jpeg_enc_job_t*>(db + hd.jobs_off);
    const uint32_t* d_huff = reinterpret_cast<const uint32_t*>(db + hd.huff_off);
    const int n_sums = (hd.n_blocks + NT - 1) / NT;
    const int rc = maf_check_hip(hipMemsetAsync(packed, 0, (size_t)hd.n_chunks * CHUNK, s), "jpeg_encode memset");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_enc_transform_kernel, dim3(n_sums), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_blocks, reinterpret_cast<const uint16_t*>(db + hd.quant_off), coef);
    MAF_LAUNCH_CHECK("jpeg_enc_transform");
    hipLaunchKernelGGL(jpeg_enc_count_kernel, dim3(n_sums), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_blocks, d_huff, coef, bits, sums);
    MAF_LAUNCH_CHECK("jpeg_enc_count");
    hipLaunchKernelGGL(jpeg_enc_sums_kernel, dim3(1), dim3(NT), 0, s, sums, n_sums);
    MAF_LAUNCH_CHECK("jpeg_enc_sums");
    hipLaunchKernelGGL(jpeg_enc_offsets_kernel, dim3(n_sums), dim3(NT), 0, s, bits, sums, n_sums, hd.n_blocks, bitoff);
    MAF_LAUNCH_CHECK("jpeg_enc_offsets");
    hipLaunchKernelGGL(jpeg_enc_pack_kernel, dim3(n_sums), dim3(NT), 0, s, d_jobs, hd.n_files, hd.n_blocks, d_huff, coef, bitoff, reinterpret_cast<uint32_t*>(packed));
    MAF_LAUNCH_CHECK("jpeg_enc_pack");
    hipLaunchKernelGGL(jpeg_enc_ffcount_kernel, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, bitoff, packed, ffcount);
    MAF_LAUNCH_CHECK("jpeg_enc_ffcount");
    hipLaunchKernelGGL(jpeg_enc_ffscan_kernel, dim3(hd.n_files), dim3(NT), 0, s, d_jobs, bitoff, ffcount, lengths);
    MAF_LAUNCH_CHECK("jpeg_enc_ffscan");
    hipLaunchKernelGGL(jpeg_enc_lenscan_kernel, dim3(1), dim3(NT), 0, s, lengths, offsets, hd.n_files);
    MAF_LAUNCH_CHECK("jpeg_enc_lenscan");
    hipLaunchKernelGGL(jpeg_enc_stuff_kernel, dim3(hd.n_chunks), dim3(NT), 0, s, d_jobs, hd.n_files, bitoff, packed, ffcount, offsets, db + hd.heads_off, out, hd.out_bytes);
    MAF_LAUNCH_CHECK("jpeg_enc_stuff");
    return 0;
}
