// BMP encoding for a batch of frames or rectangles of frames: uint8 [h][w][3] BGR in (read in place, any row pitch), 24-bit BI_RGB bottom-up
// files with a BITMAPINFOHEADER out.  Replaces the final cv2.imwrite of Inferer.infer (yolov6/core/inferer.py) for a .bmp source.  The layout
// is restated in tests/bmp_encode_ref.py; the host side (sizes, the job table) is maf-yolo_amd/bmp_encode.py; include/mafyolo_bmp_encode.h
// describes the blob and the one kernel.
#include "maf_common.h"
#include "../../include/mafyolo_bmp_encode.h"
#include "image_blob.h"

namespace {

constexpr int NT = 256;
constexpr int CHUNK = MAF_BMP_ENC_CHUNK;
constexpr int HEAD = MAF_BMP_ENC_HEAD_BYTES;
static_assert(CHUNK == 16 * NT, "a thread owns 16 aligned bytes of a chunk");

__device__ __forceinline__ int64_t row_stride(int w) { return (3 * (int64_t)w + 3) & ~(int64_t)3; }

// byte q < 54 of the file of job j: the two headers
__device__ __forceinline__ uint32_t header_byte(const maf_bmp_enc_job_t& j, int64_t stride, int64_t q) {
    const uint32_t size = (uint32_t)(HEAD + stride * j.h);
    if (q < 2) return q == 0 ? 'B' : 'M';
    if (q < 6) return (size >> (8 * (q - 2))) & 0xFFu;                           // bfSize
    if (q < 10) return 0u;                                                       // bfReserved1, bfReserved2
    if (q < 14) return q == 10 ? (uint32_t)HEAD : 0u;                            // bfOffBits
    if (q < 18) return q == 14 ? 40u : 0u;                                       // biSize
    if (q < 22) return ((uint32_t)j.w >> (8 * (q - 18))) & 0xFFu;                // biWidth
    if (q < 26) return ((uint32_t)j.h >> (8 * (q - 22))) & 0xFFu;                // biHeight, positive: bottom-up
    if (q == 26) return 1u;                                                      // biPlanes
    if (q == 28) return 24u;                                                     // biBitCount
    return 0u;                                                                   // biCompression BI_RGB, and the five DWORDs behind it
}

// the bytes [q, q + n) of the file of job j (inside the file, n <= 16) through put(i, byte): ONE division, then row and column are stepped
template <typename Put>
__device__ __forceinline__ void file_bytes(const maf_bmp_enc_job_t& j, int64_t stride, int64_t q, int n, Put put) {
    int i = 0;
    for (; i < n && q + i < HEAD; ++i) put(i, header_byte(j, stride, q + i));
    if (i == n) return;
    const int64_t r = (q + i - HEAD) / stride, live = 3 * (int64_t)j.w;
    int64_t c = (q + i - HEAD) - r * stride;
    const uint8_t* row = static_cast<const uint8_t*>(j.src) + (j.h - 1 - r) * j.pitch;      // bottom-up
    for (; i < n; ++i) {
        put(i, c < live ? (uint32_t)row[c] : 0u);                                // the row's padding is zero
        if (++c == stride) { c = 0; row -= j.pitch; }
    }
}

__global__ __launch_bounds__(NT) void bmp_enc_kernel(const maf_bmp_enc_job_t* jobs, int n_files, uint8_t* out, int64_t out_bytes, int32_t* lengths,
                                                      int64_t* offsets) {
    const int ch = blockIdx.x;
    int lo = 0, hi = n_files - 1;
    while (lo < hi) {                                                            // the last job whose first chunk is at most ch
        const int mid = (lo + hi + 1) >> 1;
        if (jobs[mid].chunk0 <= ch) lo = mid; else hi = mid - 1;
    }
    const maf_bmp_enc_job_t j = jobs[lo];
    const int64_t stride = row_stride(j.w), size = HEAD + stride * j.h;
    if (ch == j.chunk0 && threadIdx.x == 0) { lengths[lo] = (int32_t)size; offsets[lo] = j.out_off; }
    const int64_t a0 = ((j.out_off / CHUNK) + (ch - j.chunk0)) * CHUNK + 16 * threadIdx.x;      // 16 aligned bytes of out
    const int64_t first = max(a0, j.out_off), end = min(min(a0 + 16, j.out_off + size), out_bytes);
    if (first >= end) return;
    if (first == a0 && end == a0 + 16) {
        uint64_t lo8 = 0, hi8 = 0;
        file_bytes(j, stride, a0 - j.out_off, 16, [&](int i, uint32_t b) {
            if (i < 8) lo8 |= (uint64_t)b << (8 * i); else hi8 |= (uint64_t)b << (8 * (i - 8));
        });
        const u32x4_t v = {(uint32_t)lo8, (uint32_t)(lo8 >> 32), (uint32_t)hi8, (uint32_t)(hi8 >> 32)};
        *reinterpret_cast<u32x4_t*>(out + a0) = v;
    } else {
        file_bytes(j, stride, first - j.out_off, (int)(end - first), [&](int i, uint32_t b) { out[first + i] = (uint8_t)b; });      // shared with a neighbour file
    }
}

}  // namespace

extern "C" int maf_bmp_encode_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "bmp_encode_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_bmp_enc_header_t); out[1] = (int32_t)sizeof(maf_bmp_enc_job_t);
    return 0;
}

extern "C" int maf_bmp_encode(const void* blob_host, const void* blob_dev, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_bmp_enc_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && out && lengths && offsets, "bmp_encode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, out}) && maf_aligned({offsets}, 8) && maf_aligned({lengths}, 4),
                "bmp_encode: blob and out must be 16-byte aligned, offsets 8-byte, lengths 4-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_bmp_enc_header_t hd = maf_blob_header<maf_bmp_enc_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_files), "bmp_encode: 1 to 65535 files per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "bmp_encode: blob size out of range");
    MAF_REQUIRE(hd.n_chunks > 0 && hd.n_chunks < (1 << 30), "bmp_encode: chunk count out of range");
    MAF_REQUIRE(in_blob(hd.jobs_off, (int64_t)hd.n_files * (int64_t)sizeof(maf_bmp_enc_job_t), T), "bmp_encode: the job table lies outside the blob");
    const maf_bmp_enc_job_t* jobs = reinterpret_cast<const maf_bmp_enc_job_t*>(hb + hd.jobs_off);
    int64_t chunk = 0, at = 0;
    for (int i = 0; i < hd.n_files; ++i) {
        const maf_bmp_enc_job_t& j = jobs[i];
        MAF_REQUIRE(j.src, "bmp_encode: a frame's pointer is null");
        MAF_REQUIRE(j.w > 0 && j.h > 0 && j.w <= 65535 && j.h <= 65535, "bmp_encode: width and height are 1 to 65535");
        MAF_REQUIRE(j.pitch >= 3 * (int64_t)j.w, "bmp_encode: a row pitch below 3 * width");
        const int64_t size = HEAD + ((3 * (int64_t)j.w + 3) & ~(int64_t)3) * j.h;
        MAF_REQUIRE(size < MAF_BMP_ENC_MAX_FILE, "bmp_encode: a file of 2 GiB or more");
        MAF_REQUIRE(j.out_off == at, "bmp_encode: the files must follow each other without gaps");
        MAF_REQUIRE(j.n_chunks == (at + size + CHUNK - 1) / CHUNK - at / CHUNK && j.chunk0 == chunk, "bmp_encode: the files' chunks must follow each other");
        chunk += j.n_chunks;
        at += size;
        MAF_REQUIRE(chunk < (1 << 30), "bmp_encode: chunk count out of range");
    }
    MAF_REQUIRE(chunk == hd.n_chunks, "bmp_encode: the header's chunk count differs from the jobs' sum");
    MAF_REQUIRE(hd.out_bytes >= at, "bmp_encode: out is smaller than the files");
    hipLaunchKernelGGL(bmp_enc_kernel, dim3(hd.n_chunks), dim3(NT), 0, static_cast<hipStream_t>(stream),
                       reinterpret_cast<const maf_bmp_enc_job_t*>(static_cast<const uint8_t*>(blob_dev) + hd.jobs_off), hd.n_files, out, hd.out_bytes, lengths, offsets);
    MAF_LAUNCH_CHECK("bmp_enc");
    return 0;
}
