/* BMP encoding (24 bits, BI_RGB, bottom-up, BITMAPINFOHEADER) for a batch of frames or rectangles of frames: the C-ABI of csrc/bmp_encode.hip,
 * bound by hand in maf-yolo_amd/bmp_encode.py (tests/test_bmp_encode_host.py compares the prototypes below with that binding).  Compiled into
 * libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.
 *
 * One byte blob travels, copied to the device as it is: maf_bmp_enc_header_t | maf_bmp_enc_job_t [n_files].  The frames are read in place.
 * A file's size follows from its width and height, so the host places the files in out; ONE launch on `stream`, nothing synchronises:
 *   bmp_enc_kernel   one thread per 16 aligned bytes of out: the 54 header bytes, then the rows from the bottom one up, B, G, R as the frame
 *                    holds them, each padded with zeros to a multiple of 4 bytes; lengths and offsets of the files.
 */
#ifndef MAFYOLO_BMP_ENCODE_H
#define MAFYOLO_BMP_ENCODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_bmp_enc_stream_t;      /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_BMP_ENC_CHUNK 4096           /* aligned bytes of out one workgroup writes */
#define MAF_BMP_ENC_HEAD_BYTES 54        /* BITMAPFILEHEADER 14 + BITMAPINFOHEADER 40 */
#define MAF_BMP_ENC_MAX_FILE ((int64_t)1 << 31)   /* bytes of one file, exclusive */

typedef struct {
    int32_t n_files, n_chunks;
    int64_t jobs_off, total_bytes;       /* byte offsets into the blob, 16-byte aligned */
    int64_t out_bytes;                   /* size of the device buffer */
} maf_bmp_enc_header_t;

typedef struct {
    const void* src;                     /* device pointer to the first pixel (B, G, R bytes) */
    int64_t pitch;                       /* bytes between rows, >= 3 * w */
    int64_t out_off;                     /* the file's first byte in out: the files follow each other without gaps */
    int32_t w, h;
    int32_t chunk0, n_chunks;            /* the aligned chunks of out the file touches: its first and last one may be shared with a neighbour */
} maf_bmp_enc_job_t;

int maf_bmp_encode_struct_sizes(int32_t* header_job);   /* sizeof of the two structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory.  Device buffers: out uint8 [out_bytes] (16-byte aligned), lengths int32
 * [n_files], offsets int64 [n_files].  The whole HOST copy of the blob is validated before the device is touched. */
int maf_bmp_encode(const void* blob_host, const void* blob_dev, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_bmp_enc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
