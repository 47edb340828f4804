/* TIFF encoding (8-bit RGB, strips, LZW as libtiff writes it, optionally Predictor 2) for a batch of frames or rectangles of frames: the C-ABI
 * of csrc/tiff_encode.hip, bound by hand in maf-yolo_amd/tiff_encode.py (tests/test_tiff_encode_host.py compares the prototypes below with that
 * binding).  Compiled into libmafyolo_hip.so, but NOT part of the signature table of mafyolo_hip.h: this header stands on its own.
 *
 * One byte blob travels, copied to the device as it is: maf_tiff_enc_header_t | maf_tiff_enc_job_t [n_files].  The frames are read in place.
 *
 * One memset (out) and six launches on `stream`, whatever the batch holds; nothing synchronises:
 *   tiff_enc_rows_kernel     the rectangle's rows, B, G, R -> R, G, B, each row differenced (Predictor 2) unless the job says no -> raw, 16 bytes
 *                            per thread; a file's rows follow each other without gaps, so every strip is one contiguous run;
 *   tiff_enc_lzw_kernel      ONE WAVE PER STRIP, the strips of the whole batch side by side: lane 0 walks the parse (one dictionary probe per
 *                            input byte; the dictionary is 8192 open-addressed 32-bit slots in LDS), all 64 lanes fetch the input ahead of it,
 *                            clear the dictionary on a reset and store the codes (uint16: the code in bits 0 .. 11, its width - 9 in bits
 *                            12 .. 13); per strip the number of codes and of bits;
 *   tiff_enc_layout_kernel   one workgroup per file: a scan over the strips' byte counts -> every strip's offset in its file, the file's length;
 *   tiff_enc_offsets_kernel  one workgroup: a scan over the files' lengths -> the files' offsets in out;
 *   tiff_enc_pack_kernel     one workgroup per strip: a scan over the widths gives every code's bit offset; the codes are or-ed MSB first
 *                            into the zeroed output, at the strip's place in its file;
 *   tiff_enc_frame_kernel    one workgroup per file: the 8-byte header, the BitsPerSample, StripOffsets and StripByteCounts arrays, the IFD.
 */
#ifndef MAFYOLO_TIFF_ENCODE_H
#define MAFYOLO_TIFF_ENCODE_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* maf_tiff_enc_stream_t;     /* hipStream_t (maf_stream_t of mafyolo_hip.h) */

#define MAF_TIFF_ENC_CHUNK 4096          /* bytes of raw one workgroup of the rows kernel writes */
#define MAF_TIFF_ENC_TABLE 8192          /* dictionary slots of a wave (32 KB of LDS): at most 3836 are in use */
#define MAF_TIFF_ENC_MAX_STRIP (1 << 23) /* bytes of one strip, exclusive: libtiff changes its ratio formula above */
#define MAF_TIFF_ENC_MAX_FILE ((int64_t)1 << 31)   /* worst-case bytes of one file, exclusive (classic TIFF, 32-bit offsets) */

/* codes the LZW stream of n input bytes can hold: the Clear in front, at most one code per byte, a Clear per 3836 codes (the table is full),
 * a Clear per 10000 bytes (the ratio checkpoints), the EOI */
#define MAF_TIFF_ENC_CODE_BOUND(n) ((int64_t)(n) + (int64_t)(n) / 3836 + (int64_t)(n) / 10000 + 2)
/* bytes of that stream: no code is wider than 12 bits */
#define MAF_TIFF_ENC_BYTE_BOUND(n) ((12 * MAF_TIFF_ENC_CODE_BOUND(n) + 7) / 8)

typedef struct {
    int32_t n_files, n_strips, n_chunks, reserved;
    int64_t jobs_off, total_bytes;       /* byte offsets into the blob, 16-byte aligned */
    int64_t raw_bytes, code_elems, out_bytes;     /* sizes of the device buffers (codes in elements) */
} maf_tiff_enc_header_t;

typedef struct {
    const void* src;                     /* device pointer to the first pixel (B, G, R bytes) */
    int64_t pitch;                       /* bytes between rows, >= 3 * w */
    int64_t raw_off;                     /* bytes into raw, a multiple of 16 */
    int64_t code_off;                    /* elements into codes: strip k of the file owns code_slot elements from code_off + k * code_slot */
    int32_t w, h;
    int32_t rows_per_strip;              /* 1 .. h; 3 * w * rows_per_strip < MAF_TIFF_ENC_MAX_STRIP */
    int32_t predictor;                   /* 1: Predictor 2 (horizontal differencing), 0: none and no Predictor tag */
    int32_t strip0, n_strips;            /* ceil(h / rows_per_strip) */
    int32_t chunk0, n_chunks;            /* ceil(3 * w * h / MAF_TIFF_ENC_CHUNK) */
    int32_t code_slot;                   /* MAF_TIFF_ENC_CODE_BOUND(3 * w * rows_per_strip) */
    int32_t reserved;
} maf_tiff_enc_job_t;

typedef struct {
    int32_t n_codes;                     /* with the Clears and the EOI */
    int32_t bits;                        /* of the stream, without the padding of its last byte */
    uint32_t offset;                     /* of the strip in its file */
    uint32_t bytes;                      /* (bits + 7) / 8 */
} maf_tiff_enc_strip_t;

int maf_tiff_encode_struct_sizes(int32_t* header_job_strip);   /* sizeof of the three structs above (binding check) */

/* blob_host / blob_dev: the same blob in host and in device memory.  Device buffers: raw uint8 [raw_bytes], codes uint16 [code_elems], strips
 * maf_tiff_enc_strip_t [n_strips], out uint8 [out_bytes] (a multiple of 4), lengths int32 [n_files], offsets int64 [n_files].
 * The whole HOST copy of the blob is validated before the device is touched. */
int maf_tiff_encode(const void* blob_host, const void* blob_dev, uint8_t* raw, uint16_t* codes, void* strips, uint8_t* out, int32_t* lengths,
                    int64_t* offsets, maf_tiff_enc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
