// Baseline JPEG decoding (SOF0, 8 bit, Huffman, one interleaved scan) for a batch of files: file bytes in, uint8 [h][w][3] BGR frames out,
// equal to libjpeg's defaults (JDCT_ISLOW, fancy upsampling: what cv2.imread returns) bit for bit.  Replaces the cv2.imread of
// TrainValDataset.load_image (yolov6/data/datasets.py) and LoadData (yolov6/core/inferer.py).  The rules are restated in tests/jpeg_ref.py
// (its docstring lists every one with the libjpeg file it comes from); the host side (marker walk, table building) is maf-yolo_amd/jpeg.py.
//
// Progressive files (opt-in on the host) take their coefficients from jpeg_prog_entropy_kernel of jpeg_progressive.hip instead, launched by
// maf_jpeg_decode once per scan round behind jpeg_entropy_kernel; the IDCT and colour kernels below run on both kinds alike.
//
// Three kernels, one launch each for the whole batch (include/mafyolo_hip.h describes the blob and the buffers):
//   jpeg_entropy_kernel   jdhuff.c.  Divergent scalar work: one lane per restart interval, `group` (1 to 64, the host's choice: few lanes per wave while the
//                         chip has free wave slots, since the lanes of a wave diverge and serialise) decoding lanes per one-wave workgroup, the group's
//                         Huffman table set (4 x 1 424 bytes) and the zigzag order in LDS.  A code of up to 9 bits is one LDS read; longer
//                         codes walk maxcode[10..16].  The coefficient buffer is zeroed by a memset in front, so a lane stores only the
//                         nonzero coefficients.  Bit reader: a 64-bit window refilled byte by byte from aligned 8-byte loads; every byte index is clamped to the
//                         scan buffer (which ends in zero padding) AND compared with the interval's end, past which the reader feeds zeros
//                         and counts them; a lane that consumed such bits reports MAF_JPEG_ST_SHORT_SCAN.  Every loop is bounded by the
//                         (host-validated) MCU and block counts, never by stream content.
//   jpeg_idct_kernel      jidctint.c jpeg_idct_islow.  One thread per 8 x 8 block: 8 x 16-byte loads of coefficients, the two passes in
//                         registers, 8 x 8-byte stores into the component plane (neighbouring threads write neighbouring 8 bytes of a row).
//   jpeg_color_kernel     jdsample.c + jdcolor.c.  One thread per 4 output pixels of a row; the fancy upsampling is evaluated per pixel from
//                         the chroma planes (neighbours clamped to the image's own ceil(w / 2) x ceil(h / 2) samples: the edge rules of
//                         h2v*_fancy_upsample and the context rows of jdmainct.c), 12 bytes out as three 32-bit stores where aligned.  An image with an EXIF
//                         orientation of 2 to 8 in its record is written through that permutation instead, pixel by pixel (the frame of
//                         5 to 8 is [w][h][3]): the one place the baseline and the progressive chain both end.
#include "maf_common.h"
#include "jpeg_bits.h"

namespace {

__global__ __launch_bounds__(MAF_JPEG_GROUP) void jpeg_entropy_kernel(const maf_jpeg_image_t* images, const maf_jpeg_lane_t* lanes, const uint8_t* huff,
                                                                       const uint8_t* scan, int64_t scan_bytes, int group, int16_t* coef, int32_t* status) {
    __shared__ __attribute__((aligned(16))) uint8_t tabs[SET_BYTES];
    __shared__ uint8_t zz[64];
    const int tid = threadIdx.x;
    const maf_jpeg_lane_t lane = lanes[(size_t)blockIdx.x * group + min(tid, group - 1)];     // threads past `group` only help to load the tables
    {
        const int tabset = lanes[(size_t)blockIdx.x * group].tabset;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + (size_t)tabset * SET_BYTES);
        uint32_t* dst = reinterpret_cast<uint32_t*>(tabs);
        for (int i = tid; i < SET_BYTES / 4; i += MAF_JPEG_GROUP) dst[i] = src[i];
        zz[tid] = k_zigzag[tid];
    }
    __syncthreads();
    if (tid >= group || lane.image < 0 || lane.n_mcu <= 0) return;
    const maf_jpeg_image_t im = images[lane.image];
    BitReader br;
    br.buf = scan; br.pos = lane.begin; br.end = lane.end; br.last = scan_bytes - 1; br.acc = 0; br.n = 0; br.fake = 0; br.word = 0; br.widx = -1;
    int pred[3] = {0, 0, 0};
    const int nblk0 = im.mcux * im.hs * im.mcuy * im.vs, nblk1 = im.mcux * im.mcuy;
    int fault = 0;
    for (int m = lane.first_mcu; m < lane.first_mcu + lane.n_mcu && !fault; ++m) {
        const int my = m / im.mcux, mx = m - my * im.mcux;
        for (int c = 0; c < im.ncomp && !fault; ++c) {
            const int nh = c == 0 ? im.hs : 1, nv = c == 0 ? im.vs : 1;
            const int bw = im.mcux * nh;
            const int64_t cbase = im.coef_off + 64 * (int64_t)(c == 0 ? 0 : nblk0 + (c - 1) * nblk1);
            const uint8_t* dct = tabs + im.dc_tab[c] * TAB_BYTES;
            const uint8_t* act = tabs + (2 + im.ac_tab[c]) * TAB_BYTES;
            for (int v = 0; v < nv && !fault; ++v) {
                for (int h = 0; h < nh && !fault; ++h) {
                    int16_t* blk = coef + cbase + 64 * (int64_t)((my * nv + v) * bw + mx * nh + h);
                    int s = huff_decode(br, dct);
                    if (s < 0 || s > 16) { fault = MAF_JPEG_ST_BAD_CODE; break; }
                    if (s) pred[c] += huff_extend(br.get(s), s);
                    blk[0] = (int16_t)pred[c];
                    for (int k = 1; k < 64;) {
                        const int rs = huff_decode(br, act);
                        if (rs < 0) { fault = MAF_JPEG_ST_BAD_CODE; break; }
                        const int r = rs >> 4;
                        s = rs & 15;
                        if (s) {
                            k += r;
                            if (k > 63) { fault = MAF_JPEG_ST_BAD_INDEX; break; }
                            blk[zz[k]] = (int16_t)huff_extend(br.get(s), s);
                            ++k;
                        } else if (r == 15) {
                            k += 16;
                        } else {
                            break;
                        }
                    }
                }
            }
        }
    }
    if (br.fake > br.n) fault = MAF_JPEG_ST_SHORT_SCAN;         // zeros past the interval's end were consumed: whatever they decoded to, the cause is the short scan
    if (fault) atomicOr(&status[lane.image], fault);
}

// ---- jidctint.c jpeg_idct_islow (constants: jpeg_bits.h)

template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int d[8], int o[8]) {
    int z2 = d[2], z3 = d[6];
    int z1 = (z2 + z3) * FIX_0_541196100;
    int tmp2 = z1 + z3 * (-FIX_1_847759065);
    int tmp3 = z1 + z2 * FIX_0_765366865;
    z2 = d[0]; z3 = d[4];
    int tmp0 = (z2 + z3) * (1 << CONST_BITS);
    int tmp1 = (z2 - z3) * (1 << CONST_BITS);
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = d[7]; tmp1 = d[5]; tmp2 = d[3]; tmp3 = d[1];
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * FIX_1_175875602;
    tmp0 *= FIX_0_298631336; tmp1 *= FIX_2_053119869; tmp2 *= FIX_3_072711026; tmp3 *= FIX_1_501321110;
    z1 *= -FIX_0_899976223; z2 *= -FIX_2_562915447; z3 *= -FIX_1_961570560; z4 *= -FIX_0_390180644;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    o[0] = (tmp10 + tmp3 + R) >> SHIFT; o[7] = (tmp10 - tmp3 + R) >> SHIFT;
    o[1] = (tmp11 + tmp2 + R) >> SHIFT; o[6] = (tmp11 - tmp2 + R) >> SHIFT;
    o[2] = (tmp12 + tmp1 + R) >> SHIFT; o[5] = (tmp12 - tmp1 + R) >> SHIFT;
    o[3] = (tmp13 + tmp0 + R) >> SHIFT; o[4] = (tmp13 - tmp0 + R) >> SHIFT;
}

// sample_range_limit + CENTERJSAMPLE indexed with x & RANGE_MASK (jdmaster.c prepare_range_limit_table): wraps past +-512, like the table
__device__ __forceinline__ uint32_t range_limit(int x) {
    const int v = x & 1023;
    return (uint32_t)(v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896)));
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(const maf_jpeg_image_t* images, const uint16_t* quant, const int16_t* coef, uint8_t* planes) {
    const maf_jpeg_image_t im = images[blockIdx.y];
    const int nblk0 = im.mcux * im.hs * im.mcuy * im.vs, nblk1 = im.mcux * im.mcuy;
    const int total = nblk0 + (im.ncomp == 3 ? 2 * nblk1 : 0);
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int c = t < nblk0 ? 0 : (t - nblk0 < nblk1 ? 1 : 2);
    const int local = t - (c == 0 ? 0 : nblk0 + (c - 1) * nblk1);
    const int bw = c == 0 ? im.mcux * im.hs : im.mcux;
    const int by = local / bw, bx = local - by * bw;
    const u32x4_t* in = reinterpret_cast<const u32x4_t*>(coef + im.coef_off + 64 * (int64_t)t);
    const u32x4_t* qv = reinterpret_cast<const u32x4_t*>(quant + 64 * (int64_t)(im.quant + c));
    int ws[64];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                           // dequantise row r of the block
        const u32x4_t a = in[r], q = qv[r];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ws[8 * r + 2 * j] = (int)(int16_t)(a[j] & 0xFFFFu) * (int)(q[j] & 0xFFFFu);
            ws[8 * r + 2 * j + 1] = (int)(int16_t)(a[j] >> 16) * (int)(q[j] >> 16);
        }
    }
#pragma unroll
    for (int col = 0; col < 8; ++col) {                      // pass 1: columns
        int d[8], o[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) d[r] = ws[8 * r + col];
        idct_1d<CONST_BITS - PASS1_BITS>(d, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[8 * r + col] = o[r];
    }
    const int pitch = 8 * bw;
    uint8_t* dst = planes + im.plane_off + 64 * (int64_t)(c == 0 ? 0 : nblk0 + (c - 1) * nblk1) + (int64_t)(8 * by) * pitch + 8 * bx;
#pragma unroll
    for (int r = 0; r < 8; ++r) {                           // pass 2: rows
        int o[8];
        idct_1d<CONST_BITS + PASS1_BITS + 3>(&ws[8 * r], o);
        u32x2_t v;
        v[0] = range_limit(o[0]) | (range_limit(o[1]) << 8) | (range_limit(o[2]) << 16) | (range_limit(o[3]) << 24);
        v[1] = range_limit(o[4]) | (range_limit(o[5]) << 8) | (range_limit(o[6]) << 16) | (range_limit(o[7]) << 24);
        *reinterpret_cast<u32x2_t*>(dst + (int64_t)r * pitch) = v;
    }
}

// ---- jdsample.c + jdcolor.c
// the full-resolution chroma sample at (x, y) from plane p (pitch `pitch`, the image's own dw x dh samples)
__device__ __forceinline__ int chroma_at(const uint8_t* p, int pitch, int x, int y, int hs, int vs, int dw, int dh) {
    if (hs == 1) return p[(int64_t)y * pitch + x];
    if (dw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + (x >> 1)];      // h2v1_upsample / h2v2_upsample: replication
    const int i = x >> 1, odd = x & 1;
    const int nb = odd ? min(i + 1, dw - 1) : max(i - 1, 0);
    if (vs == 1) {                                           // h2v1_fancy_upsample
        const uint8_t* row = p + (int64_t)y * pitch;
        return (3 * row[i] + row[nb] + (odd ? 2 : 1)) >> 2;
    }
    const int r = y >> 1;                                    // h2v2_fancy_upsample
    const int rf = (y & 1) ? min(r + 1, dh - 1) : max(r - 1, 0);
    const uint8_t* r0 = p + (int64_t)r * pitch;
    const uint8_t* r1 = p + (int64_t)rf * pitch;
    const int cs = 3 * r0[i] + r1[i], csn = 3 * r0[nb] + r1[nb];
    return (3 * cs + csn + (odd ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const maf_jpeg_image_t* images, const uint8_t* planes, uint8_t* out) {
    const maf_jpeg_image_t im = images[blockIdx.y];
    const int w = im.w, h = im.h;
    const int qw = (w + 3) >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)qw * h) return;
    const int y = (int)(t / qw), x0 = 4 * (int)(t - (int64_t)y * qw);
    const int nblk0 = im.mcux * im.hs * im.mcuy * im.vs, nblk1 = im.mcux * im.mcuy;
    const int pitch0 = 8 * im.mcux * im.hs, pitch1 = 8 * im.mcux;
    const uint8_t* py = planes + im.plane_off;
    const uint8_t* pcb = py + 64 * (int64_t)nblk0;
    const uint8_t* pcr = pcb + 64 * (int64_t)nblk1;
    const int dw = (w + im.hs - 1) / im.hs, dh = (h + im.vs - 1) / im.vs;
    const int n = min(4, w - x0);
    uint8_t px[12];
    for (int j = 0; j < n; ++j) {
        const int x = x0 + j;
        const int yv = py[(int64_t)y * pitch0 + x];
        if (im.ncomp == 1) {
            px[3 * j] = px[3 * j + 1] = px[3 * j + 2] = (uint8_t)yv;
        } else {
            const int cb = chroma_at(pcb, pitch1, x, y, im.hs, im.vs, dw, dh) - 128;
            const int cr = chroma_at(pcr, pitch1, x, y, im.hs, im.vs, dw, dh) - 128;
            // jdcolor.c build_ycc_rgb_table: Cb_b_tab, Cb_g_tab + Cr_g_tab (ONE_HALF folded into the Cb term), Cr_r_tab
            px[3 * j] = clamp_u8(yv + ((116130 * cb + 32768) >> 16));
            px[3 * j + 1] = clamp_u8(yv + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
            px[3 * j + 2] = clamp_u8(yv + ((91881 * cr + 32768) >> 16));
        }
    }
    if (im.orientation > 1) {
        // EXIF orientation 2 to 8: the stored pixel (x, y) lands at (dx, dy) of a frame of W x H = w x h (2 to 4) or h x w (5 to 8); a
        // permutation of the same 3 * w * h bytes, pixel by pixel (the stores of 5 to 8 run down a column)
        const int ori = im.orientation;
        const bool swap = ori >= 5;
        const int W = swap ? h : w;
        for (int j = 0; j < n; ++j) {
            const int x = x0 + j;
            const int fx = (ori == 2 || ori == 3 || ori == 7 || ori == 8) ? w - 1 - x : x;      // mirrored along the stored rows
            const int fy = (ori == 3 || ori == 4 || ori == 6 || ori == 7) ? h - 1 - y : y;      // mirrored along the stored columns
            const int dx = swap ? fy : fx, dy = swap ? fx : fy;
            uint8_t* d = out + im.out_off + 3 * ((int64_t)dy * W + dx);
            d[0] = px[3 * j]; d[1] = px[3 * j + 1]; d[2] = px[3 * j + 2];
        }
        return;
    }
    const int64_t o = im.out_off + 3 * ((int64_t)y * w + x0);
    if (n == 4 && (o & 3) == 0) {
        uint32_t* d = reinterpret_cast<uint32_t*>(out + o);
        for (int k = 0; k < 3; ++k) d[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 3 * n; ++k) out[o + k] = px[k];
    }
}

}  // namespace

extern "C" int maf_jpeg_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "jpeg_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_jpeg_header_t); out[1] = (int32_t)sizeof(maf_jpeg_image_t); out[2] = (int32_t)sizeof(maf_jpeg_lane_t);
    return 0;
}

extern "C" int maf_jpeg_decode(const void* blob_host, const void* blob_dev, int16_t* coef, uint8_t* planes, uint8_t* out, int32_t* status,
                               int32_t stages, maf_stream_t stream) {
    MAF_REQUIRE(blob_host && blob_dev && coef && planes && out && status, "jpeg_decode: null pointer");
    MAF_REQUIRE(stages > 0 && (stages & ~MAF_JPEG_STAGE_ALL) == 0, "jpeg_decode: stages is a mask of MAF_JPEG_STAGE_*");
    MAF_REQUIRE(maf_aligned({blob_dev, coef, planes, out}), "jpeg_decode: buffers must be 16-byte aligned");
    const uint8_t* hb = static_cast<const uint8_t*>(blob_host);
    const maf_jpeg_header_t hd = maf_blob_header<maf_jpeg_header_t>(hb);
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(maf_blob_count_ok(hd.n_images), "jpeg_decode: 1 to 65535 images per call");
    const bool prog = hd.n_scans != 0 || hd.n_slanes != 0 || hd.n_rounds != 0;      // progressive files in the call (jpeg_progressive.hip): they have no baseline lanes
    MAF_REQUIRE(hd.group >= 1 && hd.group <= MAF_JPEG_GROUP && (prog ? hd.n_lanes >= 0 : hd.n_lanes > 0) && hd.n_lanes % hd.group == 0 && hd.n_tabsets > 0,
                "jpeg_decode: the lanes come in whole groups of 1 to MAF_JPEG_GROUP");
    MAF_REQUIRE(maf_blob_size_ok(T), "jpeg_decode: blob size out of range");
    MAF_REQUIRE(in_blob(hd.images_off, (int64_t)hd.n_images * (int64_t)sizeof(maf_jpeg_image_t), T) &&
                in_blob(hd.lanes_off, (int64_t)hd.n_lanes * (int64_t)sizeof(maf_jpeg_lane_t), T) &&
                in_blob(hd.huff_off, (int64_t)hd.n_tabsets * SET_BYTES, T) && in_blob(hd.quant_off, (int64_t)hd.n_images * 3 * 128, T) &&
                in_blob(hd.scan_off, hd.scan_bytes, T) && hd.scan_bytes >= MAF_JPEG_SCAN_PAD && hd.scan_bytes % 8 == 0, "jpeg_decode: a blob section lies outside the blob");
    MAF_REQUIRE(hd.coef_elems > 0 && hd.plane_bytes > 0 && hd.out_bytes > 0, "jpeg_decode: empty output buffers");
    const maf_jpeg_image_t* ims = reinterpret_cast<const maf_jpeg_image_t*>(hb + hd.images_off);
    const maf_jpeg_lane_t* lns = reinterpret_cast<const maf_jpeg_lane_t*>(hb + hd.lanes_off);
    int64_t max_blocks = 1, max_quads = 1;
    for (int i = 0; i < hd.n_images; ++i) {
        const maf_jpeg_image_t& m = ims[i];
        MAF_REQUIRE(m.w > 0 && m.h > 0 && m.w <= 65535 && m.h <= 65535 && (m.ncomp == 1 || m.ncomp == 3), "jpeg_decode: bad image size or component count");
        MAF_REQUIRE((m.hs == 1 && m.vs == 1) || (m.ncomp == 3 && m.hs == 2 && (m.vs == 1 || m.vs == 2)), "jpeg_decode: unsupported sampling factors");
        MAF_REQUIRE(m.mcux == (m.w + 8 * m.hs - 1) / (8 * m.hs) && m.mcuy == (m.h + 8 * m.vs - 1) / (8 * m.vs), "jpeg_decode: MCU counts do not match the image size");
        const int64_t blocks = (int64_t)m.mcux * m.mcuy * (m.hs * m.vs + (m.ncomp == 3 ? 2 : 0));
        MAF_REQUIRE(blocks < ((int64_t)1 << 24), "jpeg_decode: image too large");
        MAF_REQUIRE(m.coef_off >= 0 && m.coef_off % 64 == 0 && m.coef_off + 64 * blocks <= hd.coef_elems, "jpeg_decode: an image's coefficients lie outside the buffer");
        MAF_REQUIRE(m.plane_off >= 0 && m.plane_off % 64 == 0 && m.plane_off + 64 * blocks <= hd.plane_bytes, "jpeg_decode: an image's planes lie outside the buffer");
        MAF_REQUIRE(m.out_off >= 0 && m.out_off % 16 == 0 && m.out_off + (int64_t)3 * m.w * m.h <= hd.out_bytes, "jpeg_decode: a frame lies outside the output buffer");
        MAF_REQUIRE(m.quant >= 0 && m.quant + 3 <= 3 * hd.n_images, "jpeg_decode: quantisation table index out of range");
        MAF_REQUIRE(m.orientation >= 0 && m.orientation <= 8, "jpeg_decode: orientation is 0 (none) or an EXIF orientation 1 to 8");
        for (int c = 0; c < 3; ++c)
            MAF_REQUIRE((m.dc_tab[c] == 0 || m.dc_tab[c] == 1) && (m.ac_tab[c] == 0 || m.ac_tab[c] == 1), "jpeg_decode: Huffman table selector out of range");
        max_blocks = blocks > max_blocks ? blocks : max_blocks;
        const int64_t quads = (int64_t)((m.w + 3) / 4) * m.h;
        max_quads = quads > max_quads ? quads : max_quads;
    }
    const int64_t scan_data = hd.scan_bytes - MAF_JPEG_SCAN_PAD;
    for (int i = 0; i < hd.n_lanes; ++i) {
        const maf_jpeg_lane_t& l = lns[i];
        MAF_REQUIRE(l.tabset >= 0 && l.tabset < hd.n_tabsets && l.tabset == lns[i - i % hd.group].tabset, "jpeg_decode: the lanes of a group share one table set");
        if (l.image < 0) continue;
        MAF_REQUIRE(l.image < hd.n_images, "jpeg_decode: a lane's image index is out of range");
        MAF_REQUIRE(l.begin >= 0 && l.begin <= l.end && l.end <= scan_data, "jpeg_decode: a lane's bytes lie outside the scan buffer");
        MAF_REQUIRE(l.first_mcu >= 0 && l.n_mcu >= 0 && (int64_t)l.first_mcu + l.n_mcu <= (int64_t)ims[l.image].mcux * ims[l.image].mcuy,
                    "jpeg_decode: a lane's MCUs lie outside its image");
    }
    if (prog) {
        const int rc = maf_jpeg_progressive_validate(hb, hd);
        if (rc) return rc;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const uint8_t* db = static_cast<const uint8_t*>(blob_dev);
    const maf_jpeg_image_t* d_ims = reinterpret_cast<const maf_jpeg_image_t*>(db + hd.images_off);
    if (stages & MAF_JPEG_STAGE_ENTROPY) {
        int rc = maf_check_hip(hipMemsetAsync(coef, 0, (size_t)hd.coef_elems * sizeof(int16_t), s), "jpeg_decode memset");
        if (rc) return rc;
        rc = maf_check_hip(hipMemsetAsync(status, 0, (size_t)hd.n_images * sizeof(int32_t), s), "jpeg_decode memset");
        if (rc) return rc;
        if (hd.n_lanes > 0) {
            hipLaunchKernelGGL(jpeg_entropy_kernel, dim3(hd.n_lanes / hd.group), dim3(MAF_JPEG_GROUP), 0, s, d_ims,
                               reinterpret_cast<const maf_jpeg_lane_t*>(db + hd.lanes_off), db + hd.huff_off, db + hd.scan_off, hd.scan_bytes, hd.group, coef, status);
            MAF_LAUNCH_CHECK("jpeg_entropy");
        }
        if (prog) {
            rc = maf_jpeg_progressive_launch(hb, db, hd, coef, status, s);
            if (rc) return rc;
        }
    }
    if (stages & MAF_JPEG_STAGE_IDCT) {
        hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)((max_blocks + 255) / 256), hd.n_images), dim3(256), 0, s, d_ims,
                           reinterpret_cast<const uint16_t*>(db + hd.quant_off), coef, planes);
        MAF_LAUNCH_CHECK("jpeg_idct");
    }
    if (stages & MAF_JPEG_STAGE_COLOR) {
        hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_quads + 255) / 256), hd.n_images), dim3(256), 0, s, d_ims, planes, out);
        MAF_LAUNCH_CHECK("jpeg_color");
    }
    return 0;
}
