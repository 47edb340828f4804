/* Lossy WebP (one VP8 key frame, RFC 6386) decoding for a batch of files: the C-ABI of csrc/vp8_decode.hip, bound by hand in
 * maf-yolo_amd/webp_lossy.py (tests/test_webp_lossy_host.py compares the prototypes below with that binding).  Compiled into libmafyolo_hip.so, but
 * NOT part of the signature table of mafyolo_hip.h nor of mafyolo_webp.h: this header stands on its own.
 *
 * The host (maf-yolo_amd/webp_lossy.py) walks the RIFF chunks and reads the 10 uncompressed bytes of the `VP8 ` chunk (frame tag, start code,
 * 14 + 14 bits of size); everything behind them — the bool-coded frame header, the partition sizes, the modes, the tokens — is decoded on the
 * device.  One byte blob travels, copied to the device as it is: maf_vp8_header_t | maf_vp8_image_t [n_images] | the chunk payloads of every
 * image behind their 10 header bytes, back to back, followed by at least MAF_VP8_STREAM_PAD zero bytes.
 *
 * Stages of a call (one chain of launches on `stream`, nothing synchronises; MAF_VP8_STAGE_ALL for a decode):
 *   PARSE    per image: the frame header, the modes and the tokens of every macroblock -> the image's scratch; clears and sets status[image].
 *   RECON    inverse DCT and intra prediction -> recon: the unfiltered planes, padded to whole macroblocks.
 *   FILTER   recon copied to yuv, then the loop filter in place in yuv.
 *   CONVERT  fancy upsampling and YUV -> BGR, cropped to w x h -> out (uint8 [h][w][3] at out_off).  An image whose status is not 0 gets an
 *            all-zero frame.
 *
 * With mbw = ceil(w / 16), mbh = ceil(h / 16) and n = mbw * mbh, the scratch region of an image (scratch + scratch_off) holds, 16-byte aligned:
 *   64 words        the frame record (word 0: the filter type, 0 none / 1 simple / 2 normal)
 *   n x 32 bytes    one record per macroblock: byte 0 flags (1: 4x4-predicted, 2: inner edges are filtered, 4: skipped), 1 the 16x16 luma mode,
 *                   2 the chroma mode, 3 the filter limit (0: not filtered), 4 the interior limit, 5 the hev threshold, 8 .. 23 the sixteen
 *                   4x4 sub-modes, 24 .. 27 a mask of the blocks (bit b: block b of 24 has a non-zero coefficient)
 *   n x 384 int16   the dequantised coefficients: 16 luma, 4 U and 4 V blocks of 16 in raster order (the Y2 block already folded into the luma DCs)
 * and its plane region (recon + planes_off and yuv + planes_off, 384 n bytes each): Y [16 mbh][16 mbw], then U and V [8 mbh][8 mbw].
 */
#ifndef MAFYOLO_VP8_H
#define MAFYOLO_VP8_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_vp8_stream_t;          /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_VP8_STREAM_PAD 64
#define MAF_VP8_MAX_SIDE 16383           /* 14-bit size fields */
#define MAF_VP8_MB_RECORD 32             /* bytes of a macroblock record */
#define MAF_VP8_MB_COEFFS 384            /* int16 coefficients of a macroblock */
#define MAF_VP8_META_WORDS 64

#define MAF_VP8_ST_INPUT_EXHAUSTED 1     /* a bool needed a byte beyond the end of its partition */
#define MAF_VP8_ST_BAD_PARTITIONS 2      /* the partition size table does not fit behind the first partition, or the sizes leave the last partition empty */
#define MAF_VP8_STAGE_PARSE 1
#define MAF_VP8_STAGE_RECON 2
#define MAF_VP8_STAGE_FILTER 4
#define MAF_VP8_STAGE_CONVERT 8
#define MAF_VP8_STAGE_ALL 15

typedef struct {
    int32_t n_images, reserved;
    int64_t images_off, stream_off, stream_bytes, total_bytes;   /* byte offsets into the blob, 16-byte aligned */
    int64_t scratch_bytes, plane_bytes, out_bytes;               /* sizes of the device buffers (recon and yuv have plane_bytes each) */
} maf_vp8_header_t;

typedef struct {
    int64_t stream_begin, stream_end;    /* byte range inside the stream section: the chunk payload behind its 10 header bytes */
    int64_t scratch_off, scratch_bytes;  /* bytes, multiples of 16 */
    int64_t planes_off;                  /* bytes, a multiple of 16; 384 * mbw * mbh bytes */
    int64_t out_off;                     /* bytes, a multiple of 16; 3 * w * h bytes */
    int32_t w, h;
    int32_t first_part_bytes;            /* the frame tag's size of the first partition, at most stream_end - stream_begin */
    int32_t reserved;
} maf_vp8_image_t;

int maf_vp8_struct_sizes(int32_t* header_image);   /* sizeof of the two structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory; scratch, recon, yuv, out, status: device buffers of header.scratch_bytes,
 * header.plane_bytes (twice), header.out_bytes bytes and n_images words.  The whole HOST copy of the blob is validated (every offset, size and
 * count) before the device is touched. */
int maf_vp8_decode(const void* blob_host, const void* blob_dev, uint8_t* scratch, uint8_t* recon, uint8_t* yuv, uint8_t* out, int32_t* status,
                   int32_t stages, maf_vp8_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
