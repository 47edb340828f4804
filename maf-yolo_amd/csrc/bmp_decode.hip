// BMP decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to what Pillow's BmpImagePlugin returns, bit for bit
// (the supported set is in maf-yolo_amd/bmp.py, the C-ABI and the blob in include/mafyolo_bmp.h).  Replaces the cv2.imread of
// TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the bmp entry of IMG_FORMATS.  The rules are
// restated in tests/bmp_ref.py; the host side (headers, palette, blob) is maf-yolo_amd/bmp.py.
//
// Two kernels, one launch each for the whole batch, whatever the mix of files (the first only when the batch holds an RLE file):
//   bmp_rle_kernel       one one-wave workgroup per RLE file.  The wave zeroes the file's index plane, then walks the stream in windows of 128
//                        bytes.  Every record begins at an even offset from the start of the data and has an even length (encoded run, end of
//                        line, end of bitmap: 2 bytes; delta: 4; absolute run: 2 + its payload padded to even), so
//                          * FETCH: lane i reads the two bytes at window + 2 i and works out the record that WOULD begin there: kind, length,
//                            pixel count;
//                          * RECORD STARTS: lane i links to lane i + length / 2.  The true records are the lanes reachable from lane 0 (the
//                            carried-in record start).  Each lane keeps the 64-bit set of lanes it reaches and the lane 2^k links ahead; six
//                            rounds of pointer jumping (set |= set of the lane ahead, ahead = ahead of ahead) give lane 0 the whole chain;
//                          * POSITIONS: a wave scan over the true records turns them into (x, y): y is a prefix sum (end of line + 1, delta
//                            + dy), x a segmented prefix sum (runs and deltas add, end of line resets), both on top of the carried-in position;
//                          * STOP: a ballot finds the first record that ends the walk: end of bitmap, a position that completes the image (the
//                            last row full, or y == h: trailing records are not looked at), a record whose bytes lie past the data, a run past
//                            its row's end (clamped to it), a delta that leaves the image.  Records behind it are dead;
//                          * WRITE: runs of up to 8 pixels are written by their own lanes, all at once; the longer ones follow, the whole wave
//                            on one run (an absolute run, up to 255 pixels and so longer than a window, reads its payload straight from the
//                            stream).  Runs never overlap: the position only moves right and up.
//                        The next window begins where the last true record's link points.
//   bmp_convert_kernel   one thread per 16 output bytes of a frame (grid.y: the image): bottom-up flip, 1 / 4 bit unpacked MSB first, palette
//                        lookup (an index at or above n_colors is black), 24 bit as it is, 32 bit without its 4th byte; one 16-byte store.
//                        A 24-bit chunk inside one row whose source is 16-byte (4-byte) aligned is one (four) wide load(s).
//
// Bounded by construction (everything the RLE kernel reads is under a file's control):
//   * input: a byte index at or past the end of the file's data yields zero without a load; a record that needs such a byte is
//     MAF_BMP_ST_INPUT_EXHAUSTED and does nothing (the host validated the range to lie inside the stream section, MAF_BMP_STREAM_PAD zero bytes
//     behind it);
//   * output: a run is cut to w - x first, its row is below h (a position at or past the last pixel stops the walk), and every store is
//     compared with h * w once more;
//   * loops: every window consumes at least one record of 2 bytes or stops, so windows <= data bytes / 2 + 2; a run is at most 255 pixels.
// The convert kernel reads raw rows the host validated (h * row_bytes bytes inside the stream section) or the plane, and palette entries below
// n_colors only.  The host copy of the blob (every offset, count and range) is validated before the device is touched.
#include "maf_common.h"
#include "image_blob.h"
#include "../../include/mafyolo_bmp.h"

namespace {

enum : int { REC_RUN = 0, REC_EOL, REC_EOB, REC_DELTA, REC_ABS };
constexpr int OWN_LANE_PIXELS = 8;

__device__ __forceinline__ int rle_byte(const uint8_t* s, int64_t i, int64_t n) { return i < n ? (int)s[i] : 0; }

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int from) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, from), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), from);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// pixel j of a run: an encoded run repeats its byte (RLE4: its two nibbles in turn), an absolute run reads its payload behind the 2-byte header
__device__ __forceinline__ uint8_t run_pixel(const uint8_t* s, int64_t n, bool rle4, int kind, int64_t o, int value, int j) {
    if (kind == REC_RUN) return (uint8_t)(rle4 ? ((j & 1) ? value & 15 : value >> 4) : value);
    if (!rle4) return (uint8_t)rle_byte(s, o + 2 + j, n);
    const int b = rle_byte(s, o + 2 + (j >> 1), n);
    return (uint8_t)((j & 1) ? b & 15 : b >> 4);
}

__global__ __launch_bounds__(64) void bmp_rle_kernel(const maf_bmp_image_t* images, const int32_t* rle, const uint8_t* streams, uint8_t* planes,
                                                      int32_t* status) {
    const int lane = threadIdx.x;
    const int img = rle[blockIdx.x];
    const maf_bmp_image_t im = images[img];
    const uint8_t* s = streams + im.src_begin;
    const int64_t n = im.src_end - im.src_begin;
    const int w = im.w, h = im.h, total = w * h;               // 3 * w * h < 2^31 (host)
    const bool rle4 = im.compression == MAF_BMP_COMP_RLE4;
    uint8_t* plane = planes + im.plane_off;
    for (int i = lane; i < (total + 15) / 16; i += 64) reinterpret_cast<uint4*>(plane)[i] = make_uint4(0, 0, 0, 0);      // the plane's slot is padded to 16
    __threadfence_block();
    __syncthreads();

    int64_t pos = 0;                                           // where the next record begins (even)
    int cx = 0, cy = 0, st = 0;                                // the position in front of it, file rows; the status
    bool done = false;
    const int64_t max_windows = n / 2 + 2;
    for (int64_t it = 0; it < max_windows && !done; ++it) {
        // fetch: the record that would begin at this lane's offset
        const int64_t o = pos + 2 * lane;
        const int b0 = rle_byte(s, o, n), b1 = rle_byte(s, o + 1, n);
        int kind, len = 2, need = 2, count = 0;
        if (b0) {
            kind = REC_RUN;
            count = b0;
        } else if (b1 == 0) {
            kind = REC_EOL;
        } else if (b1 == 1) {
            kind = REC_EOB;
        } else if (b1 == 2) {
            kind = REC_DELTA;
            len = need = 4;
        } else {
            kind = REC_ABS;
            count = b1;
            const int payload = rle4 ? (b1 + 1) >> 1 : b1;
            need = 2 + payload;                                // the pad byte may be missing at the end of the file
            len = 2 + ((payload + 1) & ~1);
        }
        const bool exhausted = o + need > n;
        const int dx = kind == REC_DELTA ? rle_byte(s, o + 2, n) : 0, dy = kind == REC_DELTA ? rle_byte(s, o + 3, n) : 0;

        // record starts: the lanes reachable from lane 0
        const int next = lane + len / 2;
        int ahead = min(next, 64);                             // 64: outside the window
        uint64_t reach = 1ull << lane;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const uint64_t reach2 = shfl_u64(reach, ahead & 63);
            const int ahead2 = __shfl(ahead, ahead & 63);
            if (ahead < 64) {
                reach |= reach2;
                ahead = ahead2;
            }
        }
        const uint64_t starts = shfl_u64(reach, 0);
        const bool rec = (starts >> lane) & 1;

        // positions: (x, y) behind every true record
        const bool run = kind == REC_RUN || kind == REC_ABS;
        int sum = rec ? (run ? count : dx) : 0;
        int reset = rec && kind == REC_EOL;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int tsum = __shfl_up(sum, d), treset = __shfl_up(reset, d);
            if (lane >= d) {
                if (!reset) sum += tsum;
                reset |= treset;
            }
        }
        const int x_after = reset ? sum : cx + sum;
        const int y_after = cy + wave_inclusive_sum(rec ? (kind == REC_EOL ? 1 : dy) : 0, lane);

        // the first record that ends the walk
        int stop = 0, fault = 0;                               // stop: 1 and nothing of the record is done, 2 and it is done
        if (rec) {
            if (exhausted) { stop = 1; fault = MAF_BMP_ST_INPUT_EXHAUSTED; }
            else if (kind == REC_EOB) stop = 1;
            else if (run && x_after > w) { stop = 2; fault = MAF_BMP_ST_RUN_PAST_ROW; }
            else if (kind == REC_DELTA && (x_after > w || y_after >= h)) { stop = 1; fault = MAF_BMP_ST_DELTA_PAST_IMAGE; }
            else if (y_after >= h || (y_after == h - 1 && x_after >= w)) stop = 2;
        }
        const uint64_t stops = __ballot(stop != 0);
        const int first = stops ? __ffsll((unsigned long long)stops) - 1 : 64;

        // write
        int c = 0, base = 0;
        if (rec && run && lane <= first && stop != 1) {
            const int x0 = x_after - count;                    // 0 <= x0 <= w: an x above w is a stop in front of this lane
            c = max(0, min(count, w - x0));
            base = y_after * w + x0;                           // y_after < h: a y of h is a stop in front of this lane
            if (y_after >= h || x0 < 0 || x0 > w) c = 0;
            c = min(c, max(0, total - base));
        }
        if (c > 0 && c <= OWN_LANE_PIXELS) {
            for (int j = 0; j < c; ++j) plane[base + j] = run_pixel(s, n, rle4, kind, o, b1, j);
        }
        uint64_t rest = __ballot(c > OWN_LANE_PIXELS);
        while (rest) {
            const int i = __ffsll((unsigned long long)rest) - 1;
            rest &= rest - 1;
            const int ci = __shfl(c, i), bi = __shfl(base, i), ki = __shfl(kind, i), vi = __shfl(b1, i);
            const int64_t oi = pos + 2 * i;
            for (int j = lane; j < ci; j += 64)
                if (bi + j < total) plane[bi + j] = run_pixel(s, n, rle4, ki, oi, vi, j);
        }

        // state
        if (first < 64) {
            done = true;
            st |= __shfl(fault, first);
        } else {
            cx = __shfl(x_after, 63);
            cy = __shfl(y_after, 63);
            const int last = 63 - __clzll((long long)starts);  // lane 0 is always a start
            pos += 2 * (int64_t)__shfl(next, last);            // >= 64 lanes ahead: a link inside the window would be a start itself
        }
    }
    if (!done) st |= MAF_BMP_ST_INPUT_EXHAUSTED;               // unreachable: every window consumes a record or stops
    if (st && lane == 0) atomicOr(&status[img], st);
}

__device__ __forceinline__ uint32_t bmp_pixel(const maf_bmp_image_t& im, const uint32_t* palette, const uint8_t* streams, const uint8_t* planes, int x, int y) {
    const int yf = im.top_down ? y : im.h - 1 - y;
    int idx;
    if (im.compression != MAF_BMP_COMP_RGB) {
        idx = planes[im.plane_off + (int64_t)yf * im.w + x];
    } else {
        const uint8_t* row = streams + im.src_begin + (int64_t)yf * im.row_bytes;
        if (im.bits == 24) return (uint32_t)row[3 * x] | (uint32_t)row[3 * x + 1] << 8 | (uint32_t)row[3 * x + 2] << 16;
        if (im.bits == 32) return reinterpret_cast<const uint32_t*>(row)[x] & 0xFFFFFFu;      // src_begin and row_bytes are multiples of 4
        if (im.bits == 8) idx = row[x];
        else if (im.bits == 4) idx = (row[x >> 1] >> ((~x & 1) * 4)) & 15;
        else idx = (row[x >> 3] >> (7 - (x & 7))) & 1;
    }
    return idx < im.n_colors ? palette[im.pal + idx] : 0u;     // entries are B, G, R, 0: B in the low byte
}

// grid (16-byte chunks of the largest frame / 256, images): thread t of image i writes bytes [16 t, 16 t + 16) of its frame, the others leave
__global__ __launch_bounds__(256) void bmp_convert_kernel(const maf_bmp_image_t* images, const uint32_t* palette, const uint8_t* streams, const uint8_t* planes,
                                                           uint8_t* out) {
    const maf_bmp_image_t im = images[blockIdx.y];
    const int64_t o0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 16;
    const int64_t nbytes = (int64_t)3 * im.w * im.h;
    if (o0 >= nbytes) return;
    const int p0 = (int)(o0 / 3);
    int c = (int)(o0 - (int64_t)3 * p0), y = p0 / im.w, x = p0 - y * im.w;
    uint4* dst = reinterpret_cast<uint4*>(out + im.out_off + o0);                              // out_off is a multiple of 16, the frame's slot padded to 16
    if (im.compression == MAF_BMP_COMP_RGB && im.bits == 24 && 3 * x + c + 16 <= 3 * im.w) {    // the chunk lies in one row: a copy
        const int yf = im.top_down ? y : im.h - 1 - y;
        const uint8_t* src = streams + im.src_begin + (int64_t)yf * im.row_bytes + 3 * x + c;
        const uintptr_t a = reinterpret_cast<uintptr_t>(src);
        if ((a & 15) == 0) {
            *dst = *reinterpret_cast<const uint4*>(src);
            return;
        }
        if ((a & 3) == 0) {
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            *dst = make_uint4(s4[0], s4[1], s4[2], s4[3]);
            return;
        }
    }
    uint32_t col = bmp_pixel(im, palette, streams, planes, x, y);
    uint32_t wds[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        wds[k >> 2] |= ((col >> (8 * c)) & 255u) << (8 * (k & 3));
        if (++c == 3) {
            c = 0;
            if (++x == im.w) { x = 0; ++y; }
            if (k < 15 && y < im.h) col = bmp_pixel(im, palette, streams, planes, x, y);      // behind the last pixel: padding
        }
    }
    *dst = make_uint4(wds[0], wds[1], wds[2], wds[3]);
}

}  // namespace

extern "C" int maf_bmp_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "bmp_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_bmp_header_t); out[1] = (int32_t)sizeof(maf_bmp_image_t);
    return 0;
}

extern "C" int maf_bmp_decode(const void* blob_host, const void* blob_dev, uint8_t* planes, uint8_t* out, int32_t* status, maf_bmp_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && planes && out && status, "bmp_decode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, planes, out}), "bmp_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_bmp_header_t hd = maf_blob_header<maf_bmp_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_images), "bmp_decode: 1 to 65535 images per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "bmp_decode: blob size out of range");
    MAF_REQUIRE(hd.n_rle >= 0 && hd.n_rle <= hd.n_images, "bmp_decode: RLE image count out of range");
    MAF_REQUIRE(hd.n_palette >= 0 && hd.n_palette <= 256 * hd.n_images, "bmp_decode: palette entry count out of range");
    MAF_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_bmp_image_t), T) && in_blob(hd.rle_off, (int64_t)hd.n_rle * 4, T) &&
                in_blob(hd.palette_off, (int64_t)hd.n_palette * 4, T) && in_blob(hd.stream_off, hd.stream_bytes, T) && hd.stream_bytes >= MAF_BMP_STREAM_PAD,
                "bmp_decode: a blob section lies outside the blob");
    MAF_REQUIRE(hd.planes_bytes >= 0 && hd.out_bytes > 0 && hd.planes_bytes < ((int64_t)1 << 31) && hd.out_bytes < ((int64_t)1 << 31), "bmp_decode: output buffer sizes out of range");
    const maf_bmp_image_t* ims = reinterpret_cast<const maf_bmp_image_t*>(hb + hd.images_off);
    const int32_t* rle = reinterpret_cast<const int32_t*>(hb + hd.rle_off);
    const int64_t stream_data = hd.stream_bytes - MAF_BMP_STREAM_PAD;
    int next_rle = 0;
    int64_t max_bytes = 1;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_bmp_image_t& m = ims[i];
        MAF_REQUIRE(m.w > 0 && m.h > 0 && m.w <= MAF_BMP_MAX_SIDE && m.h <= MAF_BMP_MAX_SIDE, "bmp_decode: bad image size");
        const int64_t frame = (int64_t)3 * m.w * m.h;
        MAF_REQUIRE(frame < ((int64_t)1 << 31), "bmp_decode: a frame of 2 GiB or more");
        MAF_REQUIRE(m.bits == 1 || m.bits == 4 || m.bits == 8 || m.bits == 24 || m.bits == 32, "bmp_decode: bits per pixel is 1, 4, 8, 24 or 32");
        MAF_REQUIRE(m.compression == MAF_BMP_COMP_RGB || (m.compression == MAF_BMP_COMP_RLE8 && m.bits == 8) || (m.compression == MAF_BMP_COMP_RLE4 && m.bits == 4),
                    "bmp_decode: the compression does not go with the bit depth");
        MAF_REQUIRE(m.top_down == 0 || (m.top_down == 1 && m.compression == MAF_BMP_COMP_RGB), "bmp_decode: top_down is 0, or 1 on uncompressed rows");
        MAF_REQUIRE(m.src_begin >= 0 && m.src_begin % 16 == 0 && m.src_begin <= m.src_end && m.src_end <= stream_data, "bmp_decode: a file's data lies outside the stream section");
        MAF_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off <= hd.out_bytes && (frame + 15) / 16 * 16 <= hd.out_bytes - m.out_off,
                    "bmp_decode: a frame lies outside the output buffer");
        if (m.compression == MAF_BMP_COMP_RGB) {
            const int64_t rb = ((int64_t)m.w * m.bits + 31) / 32 * 4;
            MAF_REQUIRE(m.row_bytes == rb && m.src_end - m.src_begin == rb * m.h, "bmp_decode: row_bytes or the data size does not match the image");
        } else {
            const int64_t plane = ((int64_t)m.w * m.h + 15) / 16 * 16;
            MAF_REQUIRE(m.row_bytes == 0, "bmp_decode: an RLE image has no row_bytes");
            MAF_REQUIRE(m.plane_off >= 0 && m.plane_off % 16 == 0 && m.plane_off <= hd.planes_bytes && plane <= hd.planes_bytes - m.plane_off,
                        "bmp_decode: an index plane lies outside the planes buffer");
            MAF_REQUIRE(next_rle < hd.n_rle && rle[next_rle] == i, "bmp_decode: the RLE list does not name the RLE images in order");
            ++next_rle;
        }
        if (m.bits <= 8)
            MAF_REQUIRE(m.n_colors >= 1 && m.n_colors <= (1 << m.bits) && m.pal >= 0 && m.pal <= hd.n_palette - m.n_colors, "bmp_decode: an image's palette lies outside the palette section");
        else
            MAF_REQUIRE(m.n_colors == 0 && m.pal == 0, "bmp_decode: a 24 or 32-bit image has no palette");
        max_bytes = frame > max_bytes ? frame : max_bytes;
    }
    MAF_REQUIRE(next_rle == hd.n_rle, "bmp_decode: RLE list entries that belong to no image");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const int rc = maf_check_hip(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s), "bmp_decode memset");
    if (rc) return rc;
    const maf_bmp_image_t* dims = reinterpret_cast<const maf_bmp_image_t*>(db + hd.images_off);
    if (hd.n_rle > 0) {
        hipLaunchKernelGGL(bmp_rle_kernel, dim3(hd.n_rle), dim3(64), 0, s, dims, reinterpret_cast<const int32_t*>(db + hd.rle_off), db + hd.stream_off, planes, status);
        MAF_LAUNCH_CHECK("bmp_rle");
    }
    const unsigned chunks = (unsigned)((max_bytes + 15) / 16);
    hipLaunchKernelGGL(bmp_convert_kernel, dim3((chunks + 255) / 256, hd.n_images), dim3(256), 0, s, dims, reinterpret_cast<const uint32_t*>(db + hd.palette_off),
                       db + hd.stream_off, planes, out);
    MAF_LAUNCH_CHECK("bmp_convert");
    return 0;
}
