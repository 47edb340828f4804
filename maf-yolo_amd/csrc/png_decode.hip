// PNG decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to what cv2.imread (IMREAD_COLOR) asks libpng for,
// bit for bit (PNG is lossless: every conforming decoder gives the same samples; the conversion table is in maf-yolo_amd/png.py).  Replaces the
// cv2.imread of TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the png entries of IMG_FORMATS.
// The rules are restated in tests/png_ref.py; the host side (chunk walk, CRC-32, zlib header, blob) is maf-yolo_amd/png.py.
//
// Three kernels, one launch each for the whole batch (include/mafyolo_hip.h describes the blob and the buffers):
//   png_inflate_kernel    RFC 1951 (inflate_stream of csrc/inflate.h, which tiff_decode.hip shares; what follows describes it).  A deflate
//                         stream is one serial chain, so the batch is the parallelism: one one-wave workgroup per image.
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

#include "inflate.h"

static_assert(INFLATE_ST_INPUT_EXHAUSTED == MAF_PNG_ST_INPUT_EXHAUSTED && INFLATE_ST_BAD_BLOCK_TYPE == MAF_PNG_ST_BAD_BLOCK_TYPE &&
              INFLATE_ST_BAD_STORED_LEN == MAF_PNG_ST_BAD_STORED_LEN && INFLATE_ST_BAD_CODE_LENGTHS == MAF_PNG_ST_BAD_CODE_LENGTHS &&
              INFLATE_ST_NO_CODE == MAF_PNG_ST_NO_CODE && INFLATE_ST_DISTANCE_TOO_FAR == MAF_PNG_ST_DISTANCE_TOO_FAR &&
              INFLATE_ST_TOO_MANY_BYTES == MAF_PNG_ST_TOO_MANY_BYTES && INFLATE_ST_TOO_FEW_BYTES == MAF_PNG_ST_TOO_FEW_BYTES,
              "inflate.h reports the MAF_PNG_ST_* bits");

__global__ __launch_bounds__(64) void png_inflate_kernel(const maf_png_image_t* images, const uint8_t* streams, int64_t stream_bytes, uint8_t* inflated,
                                                          int32_t* status) {
    __shared__ InflateShared sh;
    const int lane = threadIdx.x;
    const maf_png_image_t im = images[blockIdx.x];
    const int st = inflate_stream(sh, streams, stream_bytes, im.stream_begin, im.stream_end, inflated + im.inf_off, im.inflated_size, lane);
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
