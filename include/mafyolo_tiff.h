/* TIFF 6.0 (strips; none, LZW, PackBits, Deflate) decoding for a batch of files: the C-ABI of csrc/tiff_decode.hip, bound by hand in
 * maf-yolo_amd/tiff.py (tests/test_tiff_host.py compares the prototypes below with that binding).  Compiled into libmafyolo_hip.so, but NOT
 * part of the signature table of mafyolo_hip.h: this header stands on its own.
 *
 * The host (maf-yolo_amd/tiff.py) walks the first IFD of every file; the strips are decompressed and converted on the device.  One byte blob
 * travels, copied to the device as it is: maf_tiff_header_t | maf_tiff_image_t [n_images] | maf_tiff_strip_t [n_strips] | palette entries
 * (B, G, R, 0 per entry, 8 bit) | the strips of every image back to back (a Deflate strip without its 2-byte zlib header), followed by at
 * least MAF_TIFF_STREAM_PAD zero bytes.
 *
 * Two launches on `stream`, nothing synchronises:
 *   tiff_strips_kernel    one wave per strip of the whole batch: the strip's bytes -> its rows (rows + dst_off, dst_bytes = strip rows x
 *                         row_bytes, rows padded to whole bytes).  A malformed strip sets bits of status[image] and zero-fills the rest of
 *                         its rows.
 *   tiff_convert_kernel   rows -> out: undoes predictor 2, unpacks 1 / 4 bit, WhiteIsZero, palette, gray replicated, RGB as BGR
 *                         (uint8 [h][w][3] at out_off).
 */
#ifndef MAFYOLO_TIFF_H
#define MAFYOLO_TIFF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_tiff_stream_t;         /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_TIFF_STREAM_PAD 64
#define MAF_TIFF_MAX_SIDE 65535
#define MAF_TIFF_MAX_STRIP_ROWS_BYTES 2146435072   /* 2^31 - 2^20: the rows of one strip; 64 LZW codes past its end still fit int32 */

#define MAF_TIFF_COMP_NONE 1
#define MAF_TIFF_COMP_LZW 5
#define MAF_TIFF_COMP_DEFLATE 8          /* tag values 8 and 32946 both travel as 8 */
#define MAF_TIFF_COMP_PACKBITS 32773

#define MAF_TIFF_ST_INPUT_EXHAUSTED 1    /* the strip ends (or says EOI) before its rows are full */
#define MAF_TIFF_ST_LZW_BAD_CODE 2       /* an LZW code above the next free entry, or a first code after Clear above 255 */
#define MAF_TIFF_ST_LZW_TABLE_FULL 4     /* an LZW table pushed past 4095 entries */
#define MAF_TIFF_ST_PACKBITS_OVERRUN 8   /* a PackBits literal or run byte beyond the end of the strip */
#define MAF_TIFF_ST_INFLATE_SHIFT 8      /* a Deflate strip: the MAF_PNG_ST_* bits 1 .. 128 of the inflate (but TOO_MANY_BYTES: decoding stops
                                            once the rows are full), shifted left by this */

typedef struct {
    int32_t n_images, n_strips, n_palette, reserved;
    int64_t images_off, strips_off, palette_off, stream_off, stream_bytes, total_bytes;   /* byte offsets into the blob, 16-byte aligned */
    int64_t rows_bytes, out_bytes;                                                        /* sizes of the device buffers */
} maf_tiff_header_t;

typedef struct {
    int64_t rows_off;                    /* bytes, a multiple of 16; h * row_bytes bytes */
    int64_t out_off;                     /* bytes, a multiple of 16; 3 * w * h bytes */
    int32_t w, h;
    int32_t bits;                        /* bits per sample: 1, 4 or 8 */
    int32_t spp;                         /* samples per pixel: 1 or 3 (8 bit only) */
    int32_t photometric;                 /* 0 WhiteIsZero, 1 BlackIsZero, 2 RGB, 3 palette */
    int32_t predictor;                   /* 1 none, 2 horizontal differencing (8 bit only) */
    int32_t row_bytes;                   /* ceil(w * spp * bits / 8) */
    int32_t pal;                         /* palette: the first entry, 1 << bits entries */
    int32_t first_strip, n_strips;       /* its strips in the strip table */
    int32_t rows_per_strip;              /* clamped to h */
    int32_t reserved;
} maf_tiff_image_t;

typedef struct {
    int64_t src_begin, src_end;          /* byte range inside the stream section */
    int64_t dst_off;                     /* bytes into rows: the image's rows_off + first row of the strip * row_bytes */
    int32_t dst_bytes;                   /* rows of the strip * row_bytes */
    int32_t compression;                 /* MAF_TIFF_COMP_* */
    int32_t image;
    int32_t reserved;
} maf_tiff_strip_t;

int maf_tiff_struct_sizes(int32_t* header_image_strip);   /* sizeof of the three structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory; rows, out, status: device buffers of header.rows_bytes and
 * header.out_bytes bytes and n_images words.  The whole HOST copy of the blob is validated (every offset, count and strip range) before
 * the device is touched. */
int maf_tiff_decode(const void* blob_host, const void* blob_dev, uint8_t* rows, uint8_t* out, int32_t* status, maf_tiff_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
