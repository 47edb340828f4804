/* PNG encoding (8-bit RGB, one filter type per file, deflate as zlib writes it at level 1 with Z_RLE) for a batch of frames or rectangles of
 * frames: the C-ABI of csrc/png_encode.hip, bound by hand in maf-yolo_amd/png_encode.py (tests/test_png_encode_host.py compares the prototypes
 * below with that binding).  Compiled into libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.
 *
 * One byte blob travels, copied to the device as it is: maf_png_enc_header_t | maf_png_enc_job_t [n_files].  The frames are read in place.
 *
 * Ten launches and two memsets on `stream`, whatever the batch holds; nothing synchronises:
 *   png_enc_filter_kernel   BGR -> RGB, the row filter and the type byte in front of every row -> raw (16 bytes per thread); the Adler-32 sums of
 *                           the file; per chunk of MAF_PNG_ENC_CHUNK bytes the first and the last byte that starts a run;
 *   png_enc_runs_kernel     one workgroup per file: for every chunk the last run start before it and the first one behind it;
 *   png_enc_tokens_kernel   (count) symbols per chunk under the run rule (tests/png_encode_ref.py);
 *   png_enc_symscan_kernel  one workgroup per file: the first symbol of every chunk, the symbol count of the file;
 *   png_enc_tokens_kernel   (write) the tokens (uint16: below 256 a literal, 256 + length a match at distance 1) and each block's first byte;
 *   png_enc_block_kernel    one wave per deflate block of MAF_PNG_ENC_BLOCK_SYMBOLS symbols: histograms, the three trees (trees.c, one lane),
 *                           the block type, its bit length, its code table and its header bits;
 *   png_enc_offsets_kernel  one thread per file walks its blocks (a stored block pads to a byte, so its length depends on where it starts):
 *                           bit offsets, the length of every file; then the files' offsets in the output;
 *   png_enc_emit_kernel     one workgroup per block: header bits, the symbols' codes (or the stored bytes) into the zeroed packed stream;
 *   png_enc_copy_kernel     the zlib stream and the Adler-32 into the file; the CRC-32 of every 16 bytes, moved to its place in the chunk by
 *                           x^(8 * bytes behind it) mod P and xor-ed into the file's sum (crc32_combine's rule);
 *   png_enc_frame_kernel    signature, IHDR, the IDAT length, type and CRC-32, IEND.
 */
#ifndef MAFYOLO_PNG_ENCODE_H
#define MAFYOLO_PNG_ENCODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_png_enc_stream_t;      /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_PNG_ENC_CHUNK 4096           /* bytes of the filtered stream (and of the zlib stream) one workgroup owns */
#define MAF_PNG_ENC_BLOCK_SYMBOLS 16383  /* zlib's lit_bufsize - 1 at memLevel 8 */
#define MAF_PNG_ENC_CODE_WORDS 320       /* code table of a block: 286 literal/length codes, then 30 distance codes (length << 16 | code) */
#define MAF_PNG_ENC_HEAD_WORDS 80        /* header bits of a block: 3 + 14 + 19 * 3 + 316 * 7 at the most */
#define MAF_PNG_ENC_FILE_BYTES 57        /* signature, IHDR, IDAT frame, IEND: what a file holds beside its zlib stream */

#define MAF_PNG_ENC_STORED 0
#define MAF_PNG_ENC_FIXED 1
#define MAF_PNG_ENC_DYNAMIC 2
#define MAF_PNG_ENC_UNUSED (-1)          /* a block of the worst case the file did not need */

typedef struct {
    int32_t n_files, n_chunks, n_blocks, reserved;
    int64_t jobs_off, total_bytes;       /* byte offsets into the blob, 16-byte aligned */
    int64_t raw_bytes, packed_bytes, out_bytes;   /* sizes of the device buffers */
} maf_png_enc_header_t;

typedef struct {
    const void* src;                     /* device pointer to the first pixel (B, G, R bytes) */
    int64_t pitch;                       /* bytes between rows, >= 3 * w */
    int64_t raw_off;                     /* bytes into raw and elements into tok, a multiple of 16 */
    int64_t packed_off, packed_bytes;    /* the file's part of packed: a multiple of 16 >= the bound below */
    int32_t w, h;
    int32_t filter;                      /* 0 .. 4 */
    int32_t n_raw;                       /* h * (1 + 3 * w) < 2^31 */
    int32_t chunk0, n_chunks;            /* ceil(packed_bytes / MAF_PNG_ENC_CHUNK) */
    int32_t block0, n_blocks;            /* n_raw / MAF_PNG_ENC_BLOCK_SYMBOLS + 1: the most blocks the file can have */
} maf_png_enc_job_t;

typedef struct {
    int64_t bitoff;                      /* the block's first bit in the file's zlib stream (16: behind the 78 01) */
    int32_t pos;                         /* the filtered byte its first symbol starts at */
    int32_t type;                        /* MAF_PNG_ENC_* */
    int32_t bits;                        /* its length with header, and for a stored block with padding, LEN and NLEN */
    int32_t head_bits;                   /* 3, or 3 + the trees of a dynamic block */
    int32_t n_sym;                       /* symbols without end-of-block */
    int32_t stored_len;
} maf_png_enc_block_t;

/* the zlib stream of n_raw filtered bytes takes at most n_raw + 6 * (n_raw / 16383 + 1) + 6 bytes: a block is written in the cheapest of its
 * three forms, a stored block costs 3 bits, up to 7 bits of padding, 4 bytes and its bytes (under 6 bytes beside them), and every file adds
 * 2 bytes in front and 4 behind */
#define MAF_PNG_ENC_ZBOUND(n_raw) ((int64_t)(n_raw) + 6 * ((int64_t)(n_raw) / MAF_PNG_ENC_BLOCK_SYMBOLS + 1) + 6)

int maf_png_encode_struct_sizes(int32_t* header_job_block);   /* sizeof of the three structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory.  Device buffers: raw uint8 [raw_bytes], tok uint16 [raw_bytes], chunks int32
 * [5 * n_chunks], sums uint64 [4 * n_files], blocks maf_png_enc_block_t [n_blocks], codes uint32 [MAF_PNG_ENC_CODE_WORDS * n_blocks], heads uint32
 * [MAF_PNG_ENC_HEAD_WORDS * n_blocks], packed uint8 [packed_bytes], out uint8 [out_bytes], lengths int32 [n_files], offsets int64 [n_files].
 * The whole HOST copy of the blob is validated before the device is touched. */
int maf_png_encode(const void* blob_host, const void* blob_dev, uint8_t* raw, uint16_t* tok, int32_t* chunks, uint64_t* sums, void* blocks, uint32_t* codes,
                   uint32_t* heads, uint8_t* packed, uint8_t* out, int32_t* lengths, int64_t* offsets, maf_png_enc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
