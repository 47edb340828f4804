// TIFF 6.0 decoding for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out, equal to what libtiff gives Pillow, bit for bit (the
// supported set and the conversion table are in maf-yolo_amd/tiff.py, the C-ABI and the blob in include/mafyolo_tiff.h).  Replaces the cv2.imread
// of TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py) for the tif / tiff entries of IMG_FORMATS.
// The rules are restated in tests/tiff_ref.py; the host side (IFD walk, blob) is maf-yolo_amd/tiff.py.
//
// Two kernels, one launch each for the whole batch, whatever the mix of files:
//   tiff_strips_kernel    one one-wave workgroup per strip of the whole batch, branching per strip (so per workgroup: never inside a wave) on its
//                         compression; the strip's bytes -> its rows.
//       none       a copy, 64 bytes per step.
//       PackBits   the headers are one serial chain, read wave-uniformly; the literal or the run they name moves 64 bytes per step.
//       Deflate    every strip is a zlib stream of its own: inflate_stream of csrc/inflate.h, the inflate png_decode.hip runs.  Its LDS is
//                  shared with the LZW table (a strip is one or the other).
//       LZW        MSB-first codes of 9 to 12 bits; Clear 256, EOI 257, first free entry 258; the code after a Clear adds no entry, every
//                  later one adds exactly one; the width grows when the next free entry exceeds 2^width - 2.  So between two Clears the width
//                  of the k-th code depends on k alone (codes 0 .. 253 have 9 bits, .. 765 10, .. 1789 11, the rest 12) and the bit position
//                  of every code is known ahead: the wave FETCHES 64 CODES AT ONCE, lane i the code k + i.  A ballot finds the first lane that
//                  stops the run: a Clear (the wave restarts behind it with k = 0), an EOI, a code whose bits lie past the strip, a code above
//                  the next free entry, a full table.  The n codes in front of it are decoded together:
//                    * entry e of the table is the output of code e - 1 plus the byte behind it, so the table (LDS, 4096 x 8 bytes) holds an
//                      (output offset, length) per entry and every code is a copy from earlier output of the same strip;
//                    * lengths: a literal has 1, an entry made before this fetch has its table length, an entry made BY lane j of this fetch
//                      has the length of lane j - 1 plus 1.  Those links point to lower lanes only, so six rounds of pointer jumping
//                      (shuffles) resolve every chain, the KwKwK chain of a constant image (each code names the entry made just before
//                      it) included;
//                    * output offsets: a wave prefix sum of the lengths; source offsets: the table's, or the output offset of lane j - 1;
//                    * copies: a code whose source bytes all lie in front of the fetch's first output byte (nearly all of them on pictures:
//                      an entry made in the last 64 codes is rarely named) is copied by its own lane, all such codes at once; the others (and
//                      the long ones) follow in code order, the whole wave on one code, out[q + j] = out[s + j mod (q - s)] (right for the
//                      overlap of KwKwK), with a workgroup fence and barrier before bytes written by other lanes are read.
//                  Decoding stops once the strip's rows are full (a missing EOI and trailing bytes are fine).
//   tiff_convert_kernel   one wave per row: predictor 2 undone by a wave prefix sum mod 256 per channel (64 pixels per step, the carry handed on),
//                         1 / 4 bit samples unpacked MSB first (x 255 / x 17), WhiteIsZero inverted, palette looked up, gray replicated, RGB
//                         written as BGR.
//
// Bounded by construction (everything the strips kernel reads is under a file's control):
//   * input: no read outside [src_begin, src_end) of the strip, which the host validated to lie inside the stream section (zero padding of
//     MAF_TIFF_STREAM_PAD bytes behind it: the inflate's clamp lands there); a byte index at or past src_end yields zero without a load, and an
//     LZW code that needs such a byte, a PackBits header or literal there, sets a status bit and ends the strip;
//   * output: no write outside [0, dst_bytes) of the strip's own rows: every copy length is cut to dst_bytes - position first;
//   * an LZW copy source is never at or behind the write position: table offsets are output positions of earlier codes (always below the
//     position of the code that names them), clamped again before use, and the index inside a copy is taken mod (write - source);
//   * table: a code has at most 12 bits (index < 4096); an entry index is compared with 4095 before it is written;
//   * loops: LZW fetches <= strip bits / 9 + 2 (every fetch consumes a code or ends the strip), PackBits headers <= strip bytes, copy steps
//     <= dst_bytes / 64 + 1, rows <= h.
// The host copy of the blob (every offset, count and strip range) is validated before the device is touched.  A malformed strip ends with
// status bits and a zero-filled remainder.
#include "maf_common.h"
#include "image_blob.h"
#include "../../include/mafyolo_tiff.h"

namespace {

#include "inflate.h"

struct LzwEntry {
    int32_t off, len;         // where the entry's bytes begin in the strip's output, and how many they are
};
constexpr int LZW_ENTRIES = 4096, LZW_CLEAR = 256, LZW_EOI = 257, LZW_FIRST = 258;

union StripShared {
    InflateShared inflate;
    LzwEntry lzw[LZW_ENTRIES];
};

// the width of the m-th code behind a Clear (m = 0: the code that adds no entry), and the bits of the m codes in front of it
__device__ __forceinline__ int lzw_width(int m) { return 9 + (m >= 254) + (m >= 766) + (m >= 1790); }
__device__ __forceinline__ int64_t lzw_bits_before(int m) { return 9 * (int64_t)m + max(0, m - 254) + max(0, m - 766) + max(0, m - 1790); }

__device__ __forceinline__ int wave_inclusive_sum(int v, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

enum : int { LZW_STOP_NONE = 0, LZW_STOP_INPUT, LZW_STOP_CLEAR, LZW_STOP_EOI, LZW_STOP_BAD, LZW_STOP_FULL };

// streams[begin, end) -> out[0, total); called by the whole wave with wave-uniform arguments (it holds workgroup barriers)
__device__ int lzw_strip(LzwEntry* tab, const uint8_t* streams, int64_t begin, int64_t end, uint8_t* out, int total, int lane) {
    const int64_t nbits = (end - begin) * 8;
    const int64_t max_fetches = nbits / 9 + 2;
    int st = 0, p = 0, k = 0;                                  // status, bytes produced, the index behind the last Clear of the next code
    int64_t bit = 0;                                           // the next unread bit of the strip
    int prev_off = 0, prev_len = 0;                            // the output of code k - 1 (k >= 1)
    for (int64_t it = 0; it < max_fetches && p < total && !st; ++it) {
        // fetch: lane i reads code k + i
        const int m = k + lane;
        const int wd = lzw_width(m);
        const int64_t b0 = bit + lzw_bits_before(m) - lzw_bits_before(k);
        const bool short_in = b0 + wd > nbits;
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) {                          // at most 7 + 12 bits: three bytes, those at or past `end` are zero
            const int64_t idx = begin + (b0 >> 3) + j;
            v = (v << 8) | (idx < end ? (uint32_t)streams[idx] : 0u);
        }
        const int code = (int)(v >> (24 - (int)(b0 & 7) - wd)) & ((1 << wd) - 1);
        int stop = LZW_STOP_NONE;
        if (short_in) stop = LZW_STOP_INPUT;
        else if (code == LZW_CLEAR) stop = LZW_STOP_CLEAR;
        else if (code == LZW_EOI) stop = LZW_STOP_EOI;
        else if (code >= LZW_FIRST && (m == 0 || code > 257 + m)) stop = LZW_STOP_BAD;      // 257 + m is the next free entry: KwKwK
        else if (m >= 1 && 257 + m >= LZW_ENTRIES) stop = LZW_STOP_FULL;                     // this code would add entry 257 + m
        const uint64_t stops = __ballot(stop != LZW_STOP_NONE);
        const int n = stops ? __ffsll((unsigned long long)stops) - 1 : 64;                   // the codes in front of the first stop
        const int stop_kind = __shfl(stop, n & 63);                                          // read only where n < 64
        const bool live = lane < n;

        // lengths: a root knows its length, a link is one more than the lane it points to
        const int dep = code - LZW_FIRST - k;                  // >= -1: the entry was made by lane dep + 1 of this fetch (-1: from the code before the fetch)
        const bool lit = code < LZW_CLEAR;
        int len = 0, link = -1;
        int src = 0;
        if (live) {
            if (lit) {
                len = 1;
            } else if (dep < -1) {                             // made before this fetch
                const LzwEntry e = tab[code];
                len = e.len;
                src = e.off;
            } else if (dep == -1) {
                len = prev_len + 1;
                src = prev_off;
            } else {
                len = 1;
                link = dep;                                    // dep < lane: code <= 257 + m
            }
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const int from = link >= 0 ? link : lane;
            const int len2 = __shfl(len, from), link2 = __shfl(link, from);
            if (link >= 0) {
                len += len2;
                link = link2;
            }
        }
        const int incl = wave_inclusive_sum(len, lane);
        const int pos = p + incl - len;                        // where this code's bytes go
        const int pos_dep = __shfl(pos, dep >= 0 ? dep : lane);
        if (live && !lit && dep >= 0) src = pos_dep;
        const int produced = __shfl(incl, 63);                 // lanes at and behind the stop have length 0
        // the entry this code adds: the output of the code before it plus one byte
        const int before_pos = __shfl_up(pos, 1), before_len = __shfl_up(len, 1);
        if (live && m >= 1) {                                  // 257 + m <= 4095: a full table is a stop
            LzwEntry e;
            e.off = lane == 0 ? prev_off : before_pos;
            e.len = (lane == 0 ? prev_len : before_len) + 1;
            tab[257 + m] = e;
        }
        // copies
        const int cut = live && pos < total ? min(len, total - pos) : 0;
        const bool own = cut > 0 && (lit || (cut <= 16 && src >= 0 && src + cut <= p));
        if (own) {
            if (lit) {
                out[pos] = (uint8_t)code;
            } else {
                for (int j = 0; j < cut; ++j) out[pos + j] = out[src + j];
            }
        }
        __threadfence_block();
        __syncthreads();
        uint64_t rest = __ballot(cut > 0 && !own);
        while (rest) {
            const int i = __ffsll((unsigned long long)rest) - 1;
            rest &= rest - 1;
            const int q = __shfl(pos, i), c = __shfl(cut, i);
            const int s = min(max(__shfl(src, i), 0), max(q - 1, 0));    // q >= 1: the first code of a strip is a literal
            const int D = max(q - s, 1);
            for (int j0 = 0; j0 < c; j0 += 64) {
                const int j = j0 + lane;
                if (j < c && q > 0) out[q + j] = out[s + (D >= c ? j : j % D)];
            }
            __threadfence_block();
            __syncthreads();
        }
        // state
        if (n > 0) {
            prev_off = __shfl(pos, n - 1);
            prev_len = __shfl(len, n - 1);
        }
        p = min(total, p + produced);
        bit += lzw_bits_before(k + n) - lzw_bits_before(k);
        k += n;
        if (n < 64 && p < total) {
            if (stop_kind == LZW_STOP_CLEAR) {
                bit += lzw_width(k);
                k = 0;
            } else if (stop_kind == LZW_STOP_BAD) {
                st |= MAF_TIFF_ST_LZW_BAD_CODE;
            } else if (stop_kind == LZW_STOP_FULL) {
                st |= MAF_TIFF_ST_LZW_TABLE_FULL;
            } else {
                st |= MAF_TIFF_ST_INPUT_EXHAUSTED;             // the bits ran out, or EOI in front of the last row
            }
        }
    }
    if (p < total) {
        if (!st) st |= MAF_TIFF_ST_INPUT_EXHAUSTED;
        for (int i = p + lane; i < total; i += 64) out[i] = 0;
    }
    return st;
}

__device__ int packbits_strip(const uint8_t* streams, int64_t begin, int64_t end, uint8_t* out, int total, int lane) {
    int st = 0, p = 0;
    int64_t s = begin;
    for (int64_t it = 0; it < end - begin && p < total && !st; ++it) {      // every header consumes at least one byte
        if (s >= end) break;
        const int hdr = (int8_t)streams[s++];
        if (hdr >= 0) {
            const int take = min(hdr + 1, total - p);
            const int have = (int)min((int64_t)take, end - s);
            for (int i = lane; i < have; i += 64) out[p + i] = streams[s + i];
            p += have;
            s += hdr + 1;
            if (have < take) st |= MAF_TIFF_ST_PACKBITS_OVERRUN;
        } else if (hdr != -128) {
            if (s >= end) { st |= MAF_TIFF_ST_PACKBITS_OVERRUN; break; }
            const uint8_t b = streams[s++];
            const int take = min(1 - hdr, total - p);
            for (int i = lane; i < take; i += 64) out[p + i] = b;
            p += take;
        }
    }
    if (p < total) {
        if (!st) st |= MAF_TIFF_ST_INPUT_EXHAUSTED;
        for (int i = p + lane; i < total; i += 64) out[i] = 0;
    }
    return st;
}

__device__ int raw_strip(const uint8_t* streams, int64_t begin, int64_t end, uint8_t* out, int total, int lane) {
    const int have = (int)min((int64_t)total, end - begin);
    for (int i = lane; i < total; i += 64) out[i] = i < have ? streams[begin + i] : (uint8_t)0;
    return have < total ? MAF_TIFF_ST_INPUT_EXHAUSTED : 0;
}

__global__ __launch_bounds__(64) void tiff_strips_kernel(const maf_tiff_strip_t* strips, const uint8_t* streams, int64_t stream_bytes, uint8_t* rows,
                                                          int32_t* status) {
    __shared__ StripShared sh;
    const int lane = threadIdx.x;
    const maf_tiff_strip_t sp = strips[blockIdx.x];
    uint8_t* out = rows + sp.dst_off;
    int st;
    if (sp.compression == MAF_TIFF_COMP_LZW) {
        st = lzw_strip(sh.lzw, streams, sp.src_begin, sp.src_end, out, sp.dst_bytes, lane);
    } else if (sp.compression == MAF_TIFF_COMP_DEFLATE) {
        st = inflate_stream(sh.inflate, streams, stream_bytes, sp.src_begin, sp.src_end, out, sp.dst_bytes, lane);
        st = (st & ~INFLATE_ST_TOO_MANY_BYTES) << MAF_TIFF_ST_INFLATE_SHIFT;      // decoding stops once the rows are full
    } else if (sp.compression == MAF_TIFF_COMP_PACKBITS) {
        st = packbits_strip(streams, sp.src_begin, sp.src_end, out, sp.dst_bytes, lane);
    } else {
        st = raw_strip(streams, sp.src_begin, sp.src_end, out, sp.dst_bytes, lane);
    }
    if (st && lane == 0) atomicOr(&status[sp.image], st);
}

// grid (rows of the tallest image, images): workgroup (y, i) converts row y of image i, the others leave at once
__global__ __launch_bounds__(64) void tiff_convert_kernel(const maf_tiff_image_t* images, const uint32_t* palette, const uint8_t* rows, uint8_t* out) {
    const maf_tiff_image_t im = images[blockIdx.y];
    const int y = blockIdx.x, lane = threadIdx.x;
    if (y >= im.h) return;
    const uint8_t* row = rows + im.rows_off + (int64_t)y * im.row_bytes;
    uint8_t* o = out + im.out_off + (int64_t)y * im.w * 3;
    const int bits = im.bits, spp = im.spp, ph = im.photometric;
    int carry[3] = {0, 0, 0};
    for (int x0 = 0; x0 < im.w; x0 += 64) {
        const int x = x0 + lane;
        const bool live = x < im.w;
        int s[3] = {0, 0, 0};
        if (bits == 8) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (c < spp && live) s[c] = row[(int64_t)x * spp + c];
            if (im.predictor == 2) {                           // dead lanes add 0, so lane 63 holds the row's running sum
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    if (c < spp) {
                        const int t = wave_inclusive_sum(s[c], lane) + carry[c];
                        carry[c] = __shfl(t, 63) & 255;
                        s[c] = t & 255;
                    }
                }
            }
        } else if (live) {                                     // MSB first
            const int bit = x * bits;
            s[0] = (row[bit >> 3] >> (8 - bits - (bit & 7))) & ((1 << bits) - 1);
        }
        if (!live) continue;
        uint8_t b, g, r;
        if (ph == 2) {
            b = (uint8_t)s[2]; g = (uint8_t)s[1]; r = (uint8_t)s[0];
        } else if (ph == 3) {
            const uint32_t c = palette[im.pal + s[0]];         // s[0] < 1 << bits, the entries the host validated
            b = (uint8_t)c; g = (uint8_t)(c >> 8); r = (uint8_t)(c >> 16);
        } else {
            int v = bits == 8 ? s[0] : s[0] * (255 / ((1 << bits) - 1));      // x 255 / x 17
            if (ph == 0) v = 255 - v;
            b = g = r = (uint8_t)v;
        }
        o[3 * x] = b; o[3 * x + 1] = g; o[3 * x + 2] = r;
    }
}

}  // namespace

extern "C" int maf_tiff_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "tiff_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_tiff_header_t); out[1] = (int32_t)sizeof(maf_tiff_image_t); out[2] = (int32_t)sizeof(maf_tiff_strip_t);
    return 0;
}

extern "C" int maf_tiff_decode(const void* blob_host, const void* blob_dev, uint8_t* rows, uint8_t* out, int32_t* status, maf_tiff_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && rows && out && status, "tiff_decode: null pointer");
    MAF_REQUIRE(maf_aligned({blob_dev, rows, out}), "tiff_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_tiff_header_t hd = maf_blob_header<maf_tiff_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_images), "tiff_decode: 1 to 65535 images per call");
    MAF_REQUIRE(maf_blob_size_ok(T), "tiff_decode: blob size out of range");
    MAF_REQUIRE(hd.n_strips >= hd.n_images && hd.n_strips <= (1 << 24), "tiff_decode: strip count out of range");
    MAF_REQUIRE(hd.n_palette >= 0 && hd.n_palette <= 256 * hd.n_images, "tiff_decode: palette entry count out of range");
    MAF_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_tiff_image_t), T) &&
                in_blob(hd.strips_off, (int64_t)hd.n_strips * (int64_t)sizeof(maf_tiff_strip_t), T) && in_blob(hd.palette_off, (int64_t)hd.n_palette * 4, T) &&
                in_blob(hd.stream_off, hd.stream_bytes, T) && hd.stream_bytes >= MAF_TIFF_STREAM_PAD && hd.stream_bytes % 8 == 0,
                "tiff_decode: a blob section lies outside the blob");
    MAF_REQUIRE(hd.rows_bytes > 0 && hd.out_bytes > 0 && hd.rows_bytes < ((int64_t)1 << 31) && hd.out_bytes < ((int64_t)1 << 31), "tiff_decode: output buffer sizes out of range");
    const maf_tiff_image_t* ims = reinterpret_cast<const maf_tiff_image_t*>(hb + hd.images_off);
    const maf_tiff_strip_t* sps = reinterpret_cast<const maf_tiff_strip_t*>(hb + hd.strips_off);
    const int64_t stream_data = hd.stream_bytes - MAF_TIFF_STREAM_PAD;
    int64_t next_strip = 0;
    int max_h = 1;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_tiff_image_t& m = ims[i];
        MAF_REQUIRE(m.w > 0 && m.h > 0 && m.w <= MAF_TIFF_MAX_SIDE && m.h <= MAF_TIFF_MAX_SIDE, "tiff_decode: bad image size");
        MAF_REQUIRE(m.bits == 1 || m.bits == 4 || m.bits == 8, "tiff_decode: bits per sample is 1, 4 or 8");
        MAF_REQUIRE(m.photometric >= 0 && m.photometric <= 3, "tiff_decode: photometric is 0 to 3");
        MAF_REQUIRE(m.photometric == 2 ? (m.spp == 3 && m.bits == 8) : m.spp == 1, "tiff_decode: samples per pixel do not go with the photometric");
        MAF_REQUIRE(m.photometric != 3 || m.bits != 1, "tiff_decode: a palette has 4 or 8 bits");
        MAF_REQUIRE(m.predictor == 1 || (m.predictor == 2 && m.bits == 8), "tiff_decode: predictor is 1, or 2 at 8 bits");
        const int64_t rb = ((int64_t)m.w * m.spp * m.bits + 7) / 8;
        MAF_REQUIRE(m.row_bytes == rb, "tiff_decode: row_bytes does not match the image");
        MAF_REQUIRE(m.rows_off >= 0 && m.rows_off % 16 == 0 && m.rows_off <= hd.rows_bytes && rb * m.h <= hd.rows_bytes - m.rows_off,
                    "tiff_decode: an image's rows lie outside the rows buffer");
        MAF_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off <= hd.out_bytes && (int64_t)3 * m.w * m.h <= hd.out_bytes - m.out_off,
                    "tiff_decode: a frame lies outside the output buffer");
        if (m.photometric == 3)
            MAF_REQUIRE(m.pal >= 0 && m.pal <= hd.n_palette - (1 << m.bits), "tiff_decode: an image's palette lies outside the palette section");
        MAF_REQUIRE(m.rows_per_strip >= 1 && m.rows_per_strip <= m.h, "tiff_decode: rows_per_strip out of range");
        MAF_REQUIRE(m.n_strips == (m.h + m.rows_per_strip - 1) / m.rows_per_strip && m.first_strip == next_strip && m.n_strips <= hd.n_strips - next_strip,
                    "tiff_decode: an image's strips do not tile the strip table");
        for (int j = 0; j < m.n_strips; ++j) {
            const maf_tiff_strip_t& sp = sps[next_strip + j];
            const int64_t y0 = (int64_t)j * m.rows_per_strip;
            const int64_t nrows = m.h - y0 < m.rows_per_strip ? m.h - y0 : m.rows_per_strip;
            MAF_REQUIRE(sp.image == i && sp.dst_off == m.rows_off + y0 * rb && sp.dst_bytes == nrows * rb, "tiff_decode: a strip's rows do not match its image");
            MAF_REQUIRE(nrows * rb < MAF_TIFF_MAX_STRIP_ROWS_BYTES, "tiff_decode: a strip's rows are too large");      // the LZW positions of one fetch stay inside int32
            MAF_REQUIRE(sp.src_begin >= 0 && sp.src_begin <= sp.src_end && sp.src_end <= stream_data, "tiff_decode: a strip lies outside the stream section");
            MAF_REQUIRE(sp.compression == MAF_TIFF_COMP_NONE || sp.compression == MAF_TIFF_COMP_LZW || sp.compression == MAF_TIFF_COMP_DEFLATE ||
                        sp.compression == MAF_TIFF_COMP_PACKBITS, "tiff_decode: unknown compression");
        }
        next_strip += m.n_strips;
        max_h = m.h > max_h ? m.h : max_h;
    }
    MAF_REQUIRE(next_strip == hd.n_strips, "tiff_decode: strips that belong to no image");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const int rc = maf_check_hip(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s), "tiff_decode memset");
    if (rc) return rc;
    hipLaunchKernelGGL(tiff_strips_kernel, dim3(hd.n_strips), dim3(64), 0, s, reinterpret_cast<const maf_tiff_strip_t*>(db + hd.strips_off), db + hd.stream_off,
                       hd.stream_bytes, rows, status);
    MAF_LAUNCH_CHECK("tiff_strips");
    hipLaunchKernelGGL(tiff_convert_kernel, dim3(max_h, hd.n_images), dim3(64), 0, s, reinterpret_cast<const maf_tiff_image_t*>(db + hd.images_off),
                       reinterpret_cast<const uint32_t*>(db + hd.palette_off), rows, out);
    MAF_LAUNCH_CHECK("tiff_convert");
    return 0;
}
