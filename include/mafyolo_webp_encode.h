/* Lossless WebP (VP8L) encoding for a batch of frames or rectangles of frames: the C-ABI of csrc/webp_encode.hip, bound by hand in
 * maf-yolo_amd/webp_encode.py (tests/test_webp_encode_host.py compares the prototypes below with that binding).  Compiled into
 * libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.  The stream's rules (the "profile")
 * are restated in tests/webp_encode_ref.py.
 *
 * One byte blob travels, copied to the device as it is: maf_webp_enc_header_t | maf_webp_enc_job_t [n_files] | maf_webp_enc_image_t [2 * n_files].
 * The frames are read in place.  A file holds two entropy-coded images, the predictor sub-image (image 2 f) and the residuals (image 2 f + 1);
 * from the run search on, every kernel works on images and knows nothing of files.
 *
 * Fifteen launches and three memsets on `stream`, whatever the batch holds; nothing synchronises:
 *   webp_enc_gather_kernel   BGR -> ARGB with green subtracted from red and blue (4 pixels per thread);
 *   webp_enc_modes_kernel    one workgroup per block of the predictor transform: the 14 costs, reduced across lanes and through LDS, the
 *                            winning mode -> a pixel of the sub-image;
 *   webp_enc_residual_kernel the residuals under the blocks' modes -> the pixels of the main image;
 *   webp_enc_marks_kernel    per chunk of MAF_WEBP_ENC_CHUNK pixels of an image the first and the last pixel that starts a run;
 *   webp_enc_runs_kernel     one workgroup per image: for every chunk the last run start before it and the first one behind it;
 *   webp_enc_tokens_kernel   (count) tokens per chunk under the run rule;
 *   webp_enc_symscan_kernel  one workgroup per image: the first token of every chunk, the token count of the image;
 *   webp_enc_tokens_kernel   (write) the tokens (uint32: 0x80000000 | length a copy at distance 1, else the literal's R, G, B bytes);
 *   webp_enc_hist_kernel     one workgroup per chunk of tokens and code (green + length, red, blue): a histogram in LDS, its non-zero bins
 *                            added to the image's; alpha and distance have one symbol each;
 *   webp_enc_codes_kernel    one wave per image and code: the simple code, or the length-limited tree (csrc/png_trees.h, one lane), its
 *                            code table and the bits that describe it;
 *   webp_enc_tokbits_kernel  the bits of every chunk of tokens;
 *   webp_enc_bitscan_kernel  one workgroup per image: the first bit of every chunk of tokens, the bits of the image;
 *   webp_enc_offsets_kernel  the images' first bits, the length of every file; then the files' offsets in the output;
 *   webp_enc_emit_kernel     one workgroup per chunk of tokens: the tokens' bits (and, by the first chunk, the codes' descriptions) into the
 *                            zeroed packed stream;
 *   webp_enc_copy_kernel     the payload into the file, with RIFF, WEBP, VP8L, the two sizes and the pad byte around it.
 */
#ifndef MAFYOLO_WEBP_ENCODE_H
#define MAFYOLO_WEBP_ENCODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_webp_enc_stream_t;      /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_WEBP_ENC_CHUNK 1024           /* pixels, and tokens, one workgroup owns */
#define MAF_WEBP_ENC_COPY_CHUNK 4096      /* payload bytes one workgroup of the copy kernel owns */
#define MAF_WEBP_ENC_CODES 5              /* green + length, red, blue, alpha, distance */
#define MAF_WEBP_ENC_CODE_WORDS 280       /* code table of one code: length << 16 | code (bit-reversed), 256 + 24 symbols at the most */
#define MAF_WEBP_ENC_HEAD_WORDS 64        /* description of one code: 1 + 4 + 19 * 3 + 1 + 280 * 7 = 2023 bits at the most */
#define MAF_WEBP_ENC_FILE_BYTES 20        /* RIFF, size, WEBP, VP8L, size: what a file holds beside its payload and the pad byte */
#define MAF_WEBP_ENC_LEAD_BITS 50         /* signature 8, sizes 28, alpha 1, version 3; subtract-green 3; predictor 6; the sub-image's cache bit */
#define MAF_WEBP_ENC_MAIN_BITS 3          /* no further transform, no colour cache, no entropy image */
#define MAF_WEBP_ENC_MAX_SIDE 16384
#define MAF_WEBP_ENC_MAX_COPY 4096

typedef struct {
    int32_t n_files, n_images, n_chunks, n_blocks;
    int32_t n_copy, reserved;
    int64_t jobs_off, images_off, total_bytes;   /* byte offsets into the blob, 16-byte aligned */
    int64_t px_words, packed_bytes, out_bytes;   /* sizes of the device buffers */
} maf_webp_enc_header_t;

typedef struct {
    const void* src;                     /* device pointer to the first pixel (B, G, R bytes) */
    int64_t pitch;                       /* bytes between rows, >= 3 * w */
    int64_t packed_off, packed_bytes;    /* the file's part of packed: a multiple of 16 >= the bound below */
    int32_t w, h;
    int32_t bits, bw;                    /* predictor_bits 2 .. 9; blocks per row, ceil(w / 2^bits) */
    int32_t block0, n_blocks;            /* bw * ceil(h / 2^bits) */
    int32_t copy0, n_copy;               /* ceil(packed_bytes / MAF_WEBP_ENC_COPY_CHUNK) */
} maf_webp_enc_job_t;

typedef struct {
    int64_t px_off;                      /* words into argb and px, tokens into tok; a multiple of 4 */
    int32_t n_px;                        /* w * h, or n_blocks of the file for its sub-image */
    int32_t file;
    int32_t chunk0, n_chunks;            /* ceil(n_px / MAF_WEBP_ENC_CHUNK) */
    int32_t main;                        /* 0: the predictor sub-image, 1: the residuals */
    int32_t alpha;                       /* the one alpha value of its pixels: 255, 0 */
} maf_webp_enc_image_t;

/* The payload of a file of n pixels and s predictor blocks takes at most ceil((50 + 3 + 2 * 5 * 2048 + 45 * (n + s)) / 8) bytes: a code's
 * description fits MAF_WEBP_ENC_HEAD_WORDS words, a token covers at least one pixel, and it costs at most 45 bits: three codes of at most
 * 15 bits for a literal (the alpha code has one symbol and takes no bits), 15 + 10 extra bits for a copy (the distance code likewise). */
#define MAF_WEBP_ENC_BOUND(n, s) ((50 + 3 + 2 * MAF_WEBP_ENC_CODES * 32 * MAF_WEBP_ENC_HEAD_WORDS + 45 * ((int64_t)(n) + (int64_t)(s)) + 7) / 8)

int maf_webp_encode_struct_sizes(int32_t* header_job_image);   /* sizeof of the three structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory.  Device buffers: argb, px, tok uint32 [px_words]; modes int32 [n_blocks];
 * chunks int32 [6 * n_chunks]; cbits int64 [n_chunks]; hist int32 [5 * 280 * n_images]; sums int64 [4 * n_images] (tokens, description bits,
 * token bits, first bit); cinfo int32 [8 * n_images] (the description bits of the five codes); codes uint32 [5 * MAF_WEBP_ENC_CODE_WORDS *
 * n_images]; heads uint32 [5 * MAF_WEBP_ENC_HEAD_WORDS * n_images]; packed uint8 [packed_bytes]; out uint8 [out_bytes]; lengths int32
 * [n_files]; offsets int64 [n_files].  The whole HOST copy of the blob is validated before the device is touched. */
int maf_webp_encode(const void* blob_host, const void* blob_dev, uint32_t* argb, uint32_t* px, uint32_t* tok, int32_t* modes, int32_t* chunks, int64_t* cbits,
                    int32_t* hist, int64_t* sums, int32_t* cinfo, uint32_t* codes, uint32_t* heads, uint8_t* packed, uint8_t* out, int32_t* lengths,
                    int64_t* offsets, maf_webp_enc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
