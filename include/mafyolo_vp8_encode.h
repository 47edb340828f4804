/* Lossy WebP (one VP8 key frame) encoding for a batch of frames or rectangles of frames: the C-ABI of csrc/vp8_encode.hip, bound by hand in
 * maf-yolo_amd/webp_lossy_encode.py (tests/test_webp_lossy_encode_host.py compares the prototypes below with that binding).  Compiled into
 * libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.  What is written (the "profile") is
 * restated in tests/webp_lossy_encode_ref.py.
 *
 * One byte blob travels, copied to the device as it is: maf_vp8_enc_header_t | maf_vp8_enc_job_t [n_files].  The frames are read in place.
 *
 * Five launches and one memset on `stream`, whatever the batch holds; nothing synchronises:
 *   vp8_enc_convert_kernel   a thread per chroma sample (four pixels): BGR rows (pitch, rectangles) -> the Y, U, V planes, padded to whole
 *                            macroblocks by replicating the last column and row;
 *   vp8_enc_analyse_kernel   ONE workgroup per file, a wave per macroblock row of a band of 16 rows, wave r one macroblock behind wave r - 1,
 *                            one barrier per step: the four candidate predictions from the RECONSTRUCTED neighbours and their squared errors,
 *                            then a lane per 4x4 block: forward DCT (WHT of the luma DCs), quantise, dequantise, inverse -> levels, modes,
 *                            non-zero flags and the reconstruction the next macroblocks predict from;
 *   vp8_enc_tokens_kernel    a wave per (file, token partition) and one per file for the first partition: the bool coder is one serial
 *                            chain; contexts come from the stored non-zero flags, so the partitions do not wait on each other;
 *   vp8_enc_offsets_kernel   the files' lengths from the partition sizes, their offsets in the output by a scan;
 *   vp8_enc_assemble_kernel  a workgroup per file: RIFF header, frame tag, the 7 header bytes, the first partition, the size table, the
 *                            partitions, the pad byte.
 * No flags and no spinning between workgroups.  Every store into a partition is compared with the partition's capacity, which the host sizes
 * from the proven worst case below; an overflow (impossible by that proof) sets MAF_VP8_ENC_ST_OVERFLOW and the file's length becomes 0.
 */
#ifndef MAFYOLO_VP8_ENCODE_H
#define MAFYOLO_VP8_ENCODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_vp8_enc_stream_t;       /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_VP8_ENC_MAX_SIDE 16383        /* the format's 14 bits */
#define MAF_VP8_ENC_FILE_BYTES 20         /* RIFF, size, WEBP, `VP8 `, size */
#define MAF_VP8_ENC_FRAME_BYTES 10        /* frame tag 3, start code 3, width 2, height 2 */
#define MAF_VP8_ENC_HEADER_BOOLS 1094     /* first partition in front of the modes: 29 header bools, 1056 update flags, use_skip, skip_proba 8 */
#define MAF_VP8_ENC_MODE_BOOLS 8          /* per macroblock at the most: skip 1, 16x16 flag 1, luma mode 2, chroma mode 3 */
#define MAF_VP8_ENC_FLUSH_BYTES 4         /* what the bool coder appends at the end of a partition */
#define MAF_VP8_ENC_MB_BITS 20675         /* the tokens of one macroblock at the most (webp_lossy_encode_ref.mb_worst_bits derives it) */
#define MAF_VP8_ENC_MB_LEVELS 400         /* int16 levels of a macroblock: 25 blocks (24 = Y2) of 16 in zigzag order */
#define MAF_VP8_ENC_META_WORDS 16         /* int32 per file: skipped macroblocks, status, the sizes of the first and the 8 token partitions */
#define MAF_VP8_ENC_MAX_P0 (1 << 19)      /* the frame tag holds the first partition's size in 19 bits */
#define MAF_VP8_ENC_ST_OVERFLOW 1

/* A bool costs at most 8 bits (7, in fact: the range stays above 0), so the first partition of n macroblocks takes at most this many bytes */
#define MAF_VP8_ENC_P0_BOUND(n) (MAF_VP8_ENC_HEADER_BOOLS + MAF_VP8_ENC_MODE_BOOLS * (int64_t)(n) + MAF_VP8_ENC_FLUSH_BYTES)
/* and a token partition of n macroblocks at most this many */
#define MAF_VP8_ENC_PART_BOUND(n) ((MAF_VP8_ENC_MB_BITS * (int64_t)(n) + 7) / 8 + MAF_VP8_ENC_FLUSH_BYTES)

typedef struct {
    int32_t n_files, base_q;              /* 0 .. 127 */
    int32_t level, max_chroma;            /* the loop filter's level 0 .. 63; the largest 64 * mbw * mbh of the files (the convert kernel's grid) */
    int64_t jobs_off, total_bytes;        /* byte offsets into the blob, 16-byte aligned */
    int64_t plane_bytes, n_mbs;           /* sizes of the device buffers: planes and recon; macroblocks of all files */
    int64_t part_bytes, out_bytes;
} maf_vp8_enc_header_t;

typedef struct {
    const void* src;                      /* device pointer to the first pixel (B, G, R bytes) */
    int64_t pitch;                        /* bytes between rows, >= 3 * w */
    int64_t plane_off;                    /* into planes and recon: Y [16 mbh][16 mbw], U, V [8 mbh][8 mbw]; a multiple of 16 */
    int64_t part_off, part_bytes;         /* the file's part of parts: the first partition's bound, then the token partitions' */
    int64_t mb0;                          /* its first macroblock in levels and info */
    int32_t w, h;
    int32_t mbw, mbh;
    int32_t log2_parts, reserved;         /* 0 .. 3, and 2^log2_parts <= mbh */
} maf_vp8_enc_job_t;

int maf_vp8_encode_struct_sizes(int32_t* header_job);   /* sizeof of the two structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory.  Device buffers: planes, recon uint8 [plane_bytes]; levels int16
 * [400 * n_mbs]; info uint32 [n_mbs] (bits 0 .. 24: a block has a non-zero level, 25 .. 26 the luma mode, 27 .. 28 the chroma mode, 29: no
 * level at all); meta int32 [16 * n_files]; parts uint8 [part_bytes]; out uint8 [out_bytes]; lengths int32 [n_files]; offsets int64
 * [n_files].  The whole HOST copy of the blob is validated before the device is touched. */
int maf_vp8_encode(const void* blob_host, const void* blob_dev, uint8_t* planes, uint8_t* recon, int16_t* levels, uint32_t* info, int32_t* meta, uint8_t* parts,
                   uint8_t* out, int32_t* lengths, int64_t* offsets, maf_vp8_enc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
