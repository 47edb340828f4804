// The pieces the JPEG files share (jpeg_decode.hip: baseline, jpeg_progressive.hip: progressive, jpeg_encode.hip): the Huffman table layout of
// include/mafyolo_hip.h, the zigzag order, the constants of the islow DCTs, the clamped 64-bit window bit reader and the symbol decoder of jdhuff.c.
#pragma once
#include "maf_common.h"
#include "image_blob.h"

namespace {

constexpr int TAB_BYTES = MAF_JPEG_HUFF_TABLE_BYTES;
constexpr int SET_BYTES = 4 * TAB_BYTES;
constexpr int LOOK_BITS = 9;
constexpr int OFF_MAXCODE = 2 << LOOK_BITS, OFF_VALOFF = OFF_MAXCODE + 72, OFF_HUFFVAL = OFF_VALOFF + 72;
static_assert(OFF_HUFFVAL + 256 == TAB_BYTES, "Huffman table layout");

// jutils.c jpeg_natural_order, once, in the two forms the kernels read it: k_zigzag in constant memory (the decoders copy it to LDS and
// index it with decoded values) and ZZ as compile-time indices into a register array (the encoder)
#define MAF_JPEG_NATURAL_ORDER                                                                                                      \
    {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,           \
     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63}
__constant__ uint8_t k_zigzag[64] = MAF_JPEG_NATURAL_ORDER;
constexpr int ZZ[64] = MAF_JPEG_NATURAL_ORDER;

// jidctint.c / jfdctint.c: the fixed-point constants of jpeg_idct_islow and jpeg_fdct_islow
constexpr int CONST_BITS = 13, PASS1_BITS = 2;
constexpr int FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270, FIX_0_899976223 = 7373,
              FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137, FIX_1_961570560 = 16069, FIX_2_053119869 = 16819,
              FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

struct BitReader {
    const uint8_t* buf;       // the scan buffer
    int64_t pos, end, last;   // next byte, one past the interval's last byte, the last valid index of the buffer (inside the zero padding)
    uint64_t acc;             // the low n bits are unread, most significant first
    int n;
    int fake;                 // zero bits fed past the end of the interval
    uint64_t word;            // the aligned 8 bytes of the buffer that hold byte 8 * widx ... (one global load serves 8 byte reads)
    int64_t widx;

    __device__ __forceinline__ uint32_t byte_at(int64_t i) {
        i = i < 0 ? 0 : (i > last ? last : i);             // the clamp: whatever the stream says, the index stays inside the scan buffer
        const int64_t w = i >> 3;
        if (w != widx) {
            word = reinterpret_cast<const uint64_t*>(buf)[w];   // the buffer is 16-byte aligned and a multiple of 8 bytes long
            widx = w;
        }
        return (uint32_t)(word >> (8 * (int)(i & 7))) & 0xFFu;
    }

    __device__ __forceinline__ void fill() {
        while (n <= 56) {
            uint32_t b = 0;
            if (pos < end) {
                b = byte_at(pos++);
                if (b == 0xFFu && pos < end) {
                    if (byte_at(pos) == 0) {
                        ++pos;                             // 0xFF00: a stuffed data byte 0xFF
                    } else {                               // a marker inside the interval: its data ends here (jdhuff.c feeds zeros from here on)
                        pos = end;
                        b = 0;
                        fake += 8;
                    }
                }
            } else {
                fake += 8;
            }
            acc = (acc << 8) | b;
            n += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek16() const { return (uint32_t)(acc >> (n - 16)) & 0xFFFFu; }
    __device__ __forceinline__ int get(int s) {            // s in [1, 16], n >= s
        n -= s;
        return (int)((acc >> n) & ((1u << s) - 1u));
    }
};

// one Huffman symbol from table `tab` (LDS); -1: no code matches
__device__ __forceinline__ int huff_decode(BitReader& br, const uint8_t* tab) {
    br.fill();
    const uint32_t c16 = br.peek16();
    const uint32_t e = reinterpret_cast<const uint16_t*>(tab)[c16 >> (16 - LOOK_BITS)];
    if (e) {
        br.n -= (int)(e >> 8);
        return (int)(e & 0xFFu);
    }
    const int* maxcode = reinterpret_cast<const int*>(tab + OFF_MAXCODE);
    const int* valoff = reinterpret_cast<const int*>(tab + OFF_VALOFF);
    for (int l = LOOK_BITS + 1; l <= 16; ++l) {
        const int code = (int)(c16 >> (16 - l));
        if (code <= maxcode[l]) {
            br.n -= l;
            return tab[OFF_HUFFVAL + ((valoff[l] + code) & 255)];
        }
    }
    return -1;
}

// HUFF_EXTEND of jdhuff.c
__device__ __forceinline__ int huff_extend(int r, int s) { return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r; }

}  // namespace

// jpeg_progressive.hip, called by maf_jpeg_decode: checks of the progressive sections of the host copy of the blob; one launch per round
int maf_jpeg_progressive_validate(const uint8_t* blob_host, const maf_jpeg_header_t& hd);
int maf_jpeg_progressive_launch(const uint8_t* blob_host, const uint8_t* blob_dev, const maf_jpeg_header_t& hd, int16_t* coef, int32_t* status, hipStream_t s);
