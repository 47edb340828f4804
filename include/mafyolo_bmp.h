/* BMP (BI_RGB at 1 / 4 / 8 / 24 / 32 bits, BI_RLE8, BI_RLE4, 32-bit BI_BITFIELDS in B, G, R, x order) decoding for a batch of files: the C-ABI
 * of csrc/bmp_decode.hip, bound by hand in maf-yolo_amd/bmp.py (tests/test_bmp_host.py compares the prototypes below with that binding).
 * Compiled into libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.
 *
 * The host (maf-yolo_amd/bmp.py) reads the file and DIB headers and the palette; the RLE streams are expanded and the rows converted on the
 * device.  One byte blob travels, copied to the device as it is: maf_bmp_header_t | maf_bmp_image_t [n_images] | int32 [n_rle] (the RLE images,
 * ascending) | palette entries (B, G, R, 0 per entry) | the pixel data of every file back to back (each file's on a 16-byte boundary), followed
 * by at least MAF_BMP_STREAM_PAD zero bytes.
 *
 * Two launches on `stream` at the most, nothing synchronises:
 *   bmp_rle_kernel        one wave per RLE file (skipped when the call has none): the stream -> an index plane (planes + plane_off, one byte
 *                         per pixel, h * w, in file row order, zero where the stream writes nothing).  A malformed stream sets bits of
 *                         status[image]; what follows the fault stays zero.
 *   bmp_convert_kernel    raw rows or index plane -> out: bottom-up flip, 1 / 4 bit unpacked MSB first, palette (an index at or above n_colors
 *                         is black), 24 bit copied, 32 bit without its 4th byte (uint8 [h][w][3] BGR at out_off).
 */
#ifndef MAFYOLO_BMP_H
#define MAFYOLO_BMP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_bmp_stream_t;          /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_BMP_STREAM_PAD 64
#define MAF_BMP_MAX_SIDE 65535

#define MAF_BMP_COMP_RGB 0               /* uncompressed rows (32-bit BITFIELDS files travel as this) */
#define MAF_BMP_COMP_RLE8 1
#define MAF_BMP_COMP_RLE4 2

#define MAF_BMP_ST_INPUT_EXHAUSTED 1     /* the data ends with no end-of-bitmap record before the last row is complete */
#define MAF_BMP_ST_RUN_PAST_ROW 2        /* an encoded or absolute run crosses the end of its row (clamped there) */
#define MAF_BMP_ST_DELTA_PAST_IMAGE 4    /* a delta record that leaves the image */

typedef struct {
    int32_t n_images, n_rle, n_palette, reserved;
    int64_t images_off, rle_off, palette_off, stream_off, stream_bytes, total_bytes;   /* byte offsets into the blob, 16-byte aligned */
    int64_t planes_bytes, out_bytes;                                                    /* sizes of the device buffers */
} maf_bmp_header_t;

typedef struct {
    int64_t src_begin, src_end;          /* byte range inside the stream section; src_begin is a multiple of 16 */
    int64_t plane_off;                   /* bytes into planes, a multiple of 16; h * w bytes (RLE only) */
    int64_t out_off;                     /* bytes, a multiple of 16; 3 * w * h bytes */
    int32_t w, h;
    int32_t bits;                        /* 1, 4, 8, 24 or 32 */
    int32_t compression;                 /* MAF_BMP_COMP_* */
    int32_t row_bytes;                   /* uncompressed: ceil(w * bits / 32) * 4; RLE: 0 */
    int32_t top_down;                    /* 1: the first row of the file is the top one (uncompressed only) */
    int32_t pal, n_colors;               /* palette: the first entry and how many (1 .. 1 << bits) at 1 / 4 / 8 bits, else 0, 0 */
} maf_bmp_image_t;

int maf_bmp_struct_sizes(int32_t* header_image);   /* sizeof of the two structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory; planes, out, status: device buffers of max(header.planes_bytes, 16) and
 * header.out_bytes bytes and n_images words.  The whole HOST copy of the blob is validated (every offset, count and range) before the device
 * is touched. */
int maf_bmp_decode(const void* blob_host, const void* blob_dev, uint8_t* planes, uint8_t* out, int32_t* status, maf_bmp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
