/* Lossless WebP (the VP8L bit stream) decoding for a batch of files: the C-ABI of csrc/webp_decode.hip, bound by hand in maf-yolo_amd/webp.py
 * (tests/test_webp_host.py compares the prototypes below with that binding).  These entry points are compiled into libmafyolo_hip.so but are NOT
 * part of the signature table of mafyolo_hip.h: that table stays as it is, and this header stands on its own.
 *
 * The host (maf-yolo_amd/webp.py) walks the RIFF chunks and reads the 5-byte VP8L header (signature 0x2f, 14 + 14 bits of size, alpha hint,
 * version); everything behind it is inside the bit stream and is decoded on the device.  One byte blob travels, copied to the device as it
 * is: maf_webp_header_t | maf_webp_image_t [n_images] | the VP8L payloads of every image behind their 5 header bytes, back to back, followed
 * by at least MAF_WEBP_STREAM_PAD zero bytes (the section is a multiple of 8 bytes long).
 *
 * Stages of a call (one chain of launches on `stream`, nothing synchronises; MAF_WEBP_STAGE_ALL for a decode):
 *   ENTROPY    per image: the transform headers, every sub-image (predictor modes, colour-transform elements, palette, entropy image), all prefix
 *              codes, the main image -> argb (uint32 ARGB, h rows of the CODED width, at argb_off) and status[image]; clears the status words.
 *   TRANSFORM  the inverse transforms in the reverse of their reading order, into the scratch (argb is left as the ENTROPY stage wrote it).
 *   CONVERT    alpha dropped, BGR -> out (uint8 [h][w][3] at out_off).  An image whose status is not 0 gets an all-zero frame.
 *
 * The scratch region of an image (scratch + scratch_off, scratch_bytes long) holds, in this order, all 16-byte aligned:
 *   64 words       the transform record the ENTROPY stage leaves for the later stages
 *   256 words      the palette
 *   3 x S words    predictor modes, colour-transform elements, entropy image; S = ceil(w / 4) * ceil(h / 4) (a sub-image is at least 4-fold subsampled)
 *   2 x w * h words  the image behind the inverse transforms (argb keeps the ENTROPY stage's pixels; colour indexing, which widens rows, moves
 *                  from one buffer to the other)
 *   dir_words      one word per prefix code: where its record begins in the arena
 *   arena_units    uint16 units: per code 18 units (kind, the count of every length 1 .. 15, the symbol of a one-symbol code, 0), then the
 *                  code's symbols ordered by (length, symbol) unless the code has one symbol or its symbols are 0 .. 2^l - 1 in order.
 * The number of code groups is known only after the entropy image is decoded, so the host sizes both from the stream length alone
 * (MAF_WEBP_DIR_WORDS, MAF_WEBP_ARENA_UNITS), by these facts: a code costs at least 4 stream bits (a simple code of one 1-bit symbol), so n
 * stream bytes hold at most 2 n codes; a stored symbol costs at least a third of a bit (a code-length token of at least 1 bit gives one
 * length, a repeat token 16 of at least 2 bits up to 6 lengths; where the code-length code has ONE symbol its tokens cost no bits, but then
 * every used symbol has the same length l and the symbols are 0 .. 2^l - 1 in order, which is the form that stores none), so n bytes hold at
 * most 24 n stored symbols beside 2 n x 18 units of records.  A stream that still asks for more sets MAF_WEBP_ST_TABLE_SPACE.
 */
#ifndef MAFYOLO_WEBP_H
#define MAFYOLO_WEBP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_webp_stream_t;         /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_WEBP_STREAM_PAD 64
#define MAF_WEBP_MAX_SIDE 16384          /* 14-bit size fields */
#define MAF_WEBP_DIR_WORDS(stream_bytes) (2 * (stream_bytes) + 40)
#define MAF_WEBP_ARENA_UNITS(stream_bytes) (64 * (stream_bytes) + 64)

#define MAF_WEBP_ST_INPUT_EXHAUSTED 1    /* bits past the end of the image's stream were consumed (whatever else was met after that) */
#define MAF_WEBP_ST_BAD_TRANSFORM 2      /* a transform type a second time */
#define MAF_WEBP_ST_BAD_CACHE_BITS 4     /* colour cache bits outside 1 .. 11 */
#define MAF_WEBP_ST_BAD_CODE_LENGTHS 8   /* an over-subscribed or incomplete code, max_symbol above the alphabet, a run past the alphabet, a simple symbol outside it */
#define MAF_WEBP_ST_NO_CODE 16           /* no code matches the bits */
#define MAF_WEBP_ST_DISTANCE_TOO_FAR 32  /* a distance larger than the pixels produced so far */
#define MAF_WEBP_ST_COPY_PAST_END 64     /* a copy longer than the pixels left */
#define MAF_WEBP_ST_TABLE_SPACE 128      /* more codes or code symbols than the scratch was sized for */
#define MAF_WEBP_STAGE_ENTROPY 1
#define MAF_WEBP_STAGE_TRANSFORM 2
#define MAF_WEBP_STAGE_CONVERT 4
#define MAF_WEBP_STAGE_ALL 7

typedef struct {
    int32_t n_images, reserved;
    int64_t images_off, stream_off, stream_bytes, total_bytes;   /* byte offsets into the blob, 16-byte aligned */
    int64_t argb_words, scratch_bytes, out_bytes;                /* sizes of the three device buffers */
} maf_webp_header_t;

typedef struct {
    int64_t stream_begin, stream_end;    /* byte range inside the stream section: the VP8L payload behind its 5 header bytes */
    int64_t argb_off;                    /* in uint32 words, a multiple of 4; w * h words */
    int64_t scratch_off, scratch_bytes;  /* bytes, multiples of 16 */
    int64_t out_off;                     /* bytes, a multiple of 16; 3 * w * h bytes */
    int32_t w, h, dir_words, arena_units;
} maf_webp_image_t;

int maf_webp_struct_sizes(int32_t* header_image);   /* sizeof of the two structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory; argb, scratch, out, status: device buffers of header.argb_words words,
 * header.scratch_bytes bytes, header.out_bytes bytes and n_images words.  The whole HOST copy of the blob is validated (every offset, size and
 * count) before the device is touched. */
int maf_webp_decode(const void* blob_host, const void* blob_dev, uint32_t* argb, uint8_t* scratch, uint8_t* out, int32_t* status,
                    int32_t stages, maf_webp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
