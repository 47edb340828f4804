// Progressive JPEG entropy decoding (SOF2, 8 bit, Huffman) for a batch of files: jdphuff.c restated.  The host (maf-yolo_amd/jpeg.py
// parse(progressive=True)) walks and validates every scan of every file; the finished coefficients go through jpeg_idct_kernel and
// jpeg_color_kernel of jpeg_decode.hip unchanged.  The rules are restated in tests/jpeg_progressive_ref.py (its docstring lists every one);
// include/mafyolo_hip.h describes the scan table, the scan lanes and the rounds.
//
// One kernel, jpeg_prog_entropy_kernel, launched once per ROUND: round k decodes the k-th scan of every image of the call that has one.  The
// scans of one image depend on each other in order (a refinement scan reads what the scans before it wrote), so the rounds follow each other
// on the stream and nothing else orders them; scans of different images are independent, so a round is one launch whatever the batch (10
// launches for libjpeg's default script, 6 for gray).  The layout follows jpeg_entropy_kernel: divergent scalar-style work, one lane per
// (scan, restart interval), `sgroup` lanes per one-wave workgroup (the host packs few lanes per wave while the chip has free wave slots,
// since the lanes of a wave diverge and serialise), the group's Huffman table set and the zigzag order in LDS, the clamped 64-bit window bit
// reader of jpeg_bits.h.  The four routines:
//   decode_mcu_DC_first    coef[0] = (pred + diff) << Al; interleaved MCU order as in baseline (or one block per MCU in a one-component
//                          scan); the prediction starts at 0 in every lane (= at every restart)
//   decode_mcu_DC_refine   one raw bit per block: coef[0] |= 1 << Al
//   decode_mcu_AC_first    run/size symbols over Ss..Se; size 0 with run < 15 starts an EOB run of (1 << r) + get(r) blocks (this one
//                          included), run 15 is ZRL; values << Al
//   decode_mcu_AC_refine   a symbol names a new +-1 << Al coefficient and how many STILL-ZERO positions to skip before it; every already
//                          nonzero coefficient passed on the way takes one correction bit (added as +-(1 << Al) by sign, only when that bit
//                          is not set yet); during an EOB run the blocks still take the correction bits of their whole band
// EOBRUN is lane state and starts at 0 in every lane.  A block's coefficients are read, modified and written by the one lane that owns the
// block in this scan, with ordinary loads and stores.  Every loop is bounded by the host-validated MCU counts and by the 64 coefficients of
// a block, never by stream content: EOBRUN only ever says "skip the symbol decode of this block", it is never a loop bound, so a run longer
// than the blocks the lane still owns simply ends with the lane.  A position past Se sets MAF_JPEG_ST_REFINE_PAST_SE (libjpeg would write
// into the next band) and ends the lane.
#include "maf_common.h"
#include "jpeg_bits.h"

namespace {

__device__ __forceinline__ int get_bits(BitReader& br, int s) {          // s in [1, 16]
    if (br.n < s) br.fill();
    return br.get(s);
}

__global__ __launch_bounds__(MAF_JPEG_GROUP) void jpeg_prog_entropy_kernel(const maf_jpeg_image_t* images, const maf_jpeg_scan_t* scans,
                                                                            const maf_jpeg_lane_t* lanes, const uint8_t* huff, const uint8_t* scan,
                                                                            int64_t scan_bytes, int group, int16_t* coef, int32_t* status) {
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
    const maf_jpeg_scan_t sc = scans[lane.image];            // a scan lane's `image` field is its row of the scan table
    const maf_jpeg_image_t im = images[sc.image];
    BitReader br;
    br.buf = scan; br.pos = lane.begin; br.end = lane.end; br.last = scan_bytes - 1; br.acc = 0; br.n = 0; br.fake = 0; br.word = 0; br.widx = -1;
    const int nblk0 = im.mcux * im.hs * im.mcuy * im.vs, nblk1 = im.mcux * im.mcuy;
    const int al = sc.al;
    int fault = 0;
    if (sc.ss == 0) {                                        // ---- DC scans
        int pred[3] = {0, 0, 0};
        const bool inter = sc.ncomp > 1;
        for (int m = lane.first_mcu; m < lane.first_mcu + lane.n_mcu && !fault; ++m) {
            const int my = m / sc.bw, mx = m - my * sc.bw;   // the frame's MCU grid when interleaved, else the component's own block grid
            for (int j = 0; j < sc.ncomp && !fault; ++j) {
                const int c = sc.comp[j];
                const int nh = inter && c == 0 ? im.hs : 1, nv = inter && c == 0 ? im.vs : 1;
                const int pitch = c == 0 ? im.mcux * im.hs : im.mcux;       // blocks per row of the padded coefficient plane
                const int64_t cbase = im.coef_off + 64 * (int64_t)(c == 0 ? 0 : nblk0 + (c - 1) * nblk1);
                const uint8_t* dct = tabs + sc.dc_tab[j] * TAB_BYTES;
                for (int v = 0; v < nv && !fault; ++v) {
                    for (int h = 0; h < nh && !fault; ++h) {
                        int16_t* blk = coef + cbase + 64 * (int64_t)((my * nv + v) * pitch + mx * nh + h);
                        if (sc.ah == 0) {                    // decode_mcu_DC_first
                            const int s = huff_decode(br, dct);
                            if (s < 0 || s > 16) { fault = MAF_JPEG_ST_BAD_CODE; break; }
                            if (s) pred[j] += huff_extend(br.get(s), s);
                            blk[0] = (int16_t)((uint32_t)pred[j] << al);
                        } else if (get_bits(br, 1)) {        // decode_mcu_DC_refine
                            blk[0] = (int16_t)(blk[0] | (1 << al));
                        }
                    }
                }
            }
        }
    } else {                                                 // ---- AC scans: one component, one block per MCU
        const int c = sc.comp[0];
        const int pitch = c == 0 ? im.mcux * im.hs : im.mcux;
        const int64_t cbase = im.coef_off + 64 * (int64_t)(c == 0 ? 0 : nblk0 + (c - 1) * nblk1);
        const uint8_t* act = tabs + (2 + sc.ac_tab) * TAB_BYTES;
        const int ss = sc.ss, se = sc.se;
        const int p1 = 1 << al, m1 = -(1 << al);
        int eobrun = 0;
        for (int m = lane.first_mcu; m < lane.first_mcu + lane.n_mcu && !fault; ++m) {
            const int by = m / sc.bw, bx = m - by * sc.bw;
            int16_t* blk = coef + cbase + 64 * (int64_t)(by * pitch + bx);
            if (sc.ah == 0) {                                // decode_mcu_AC_first
                if (eobrun > 0) { --eobrun; continue; }
                for (int k = ss; k <= se; ++k) {
                    const int rs = huff_decode(br, act);
                    if (rs < 0) { fault = MAF_JPEG_ST_BAD_CODE; break; }
                    const int r = rs >> 4, s = rs & 15;
                    if (s) {
                        k += r;
                        if (k > se) { fault = k > 63 ? MAF_JPEG_ST_BAD_INDEX : MAF_JPEG_ST_REFINE_PAST_SE; break; }
                        blk[zz[k]] = (int16_t)((uint32_t)huff_extend(br.get(s), s) << al);
                    } else if (r == 15) {
                        k += 15;                             // ZRL: 16 zeros with the loop's own step
                    } else {
                        eobrun = 1 << r;                     // EOBr: this block and eobrun - 1 more end here
                        if (r) eobrun += br.get(r);
                        --eobrun;
                        break;
                    }
                }
            } else {                                         // decode_mcu_AC_refine
                int k = ss;
                if (eobrun == 0) {
                    for (; k <= se; ++k) {
                        const int rs = huff_decode(br, act);
                        if (rs < 0) { fault = MAF_JPEG_ST_BAD_CODE; break; }
                        int r = rs >> 4, s = rs & 15;
                        if (s) {
                            if (s != 1) { fault = MAF_JPEG_ST_BAD_CODE; break; }     // size must be 1 (JWRN_HUFF_BAD_CODE)
                            s = br.get(1) ? p1 : m1;
                        } else if (r != 15) {
                            eobrun = 1 << r;
                            if (r) eobrun += br.get(r);
                            break;                           // the rest of the band is handled as the first block of the EOB run
                        }
                        do {                                 // skip r still-zero positions (all 16 of a ZRL), correcting the nonzero ones passed
                            const int z = zz[k];
                            const int v = blk[z];
                            if (v != 0) {
                                if (get_bits(br, 1) && (v & p1) == 0) blk[z] = (int16_t)(v + (v >= 0 ? p1 : m1));
                            } else if (--r < 0) {
                                break;
                            }
                            ++k;
                        } while (k <= se);
                        if (s) {
                            if (k > se) { fault = MAF_JPEG_ST_REFINE_PAST_SE; break; }
                            blk[zz[k]] = (int16_t)s;
                        }
                    }
                }
                if (eobrun > 0 && !fault) {                  // inside an EOB run: the remaining nonzero coefficients of the band take their correction bits
                    for (; k <= se; ++k) {
                        const int z = zz[k];
                        const int v = blk[z];
                        if (v != 0 && get_bits(br, 1) && (v & p1) == 0) blk[z] = (int16_t)(v + (v >= 0 ? p1 : m1));
                    }
                    --eobrun;
                }
            }
        }
    }
    if (br.fake > br.n) fault = MAF_JPEG_ST_SHORT_SCAN;         // zeros past the interval's end were consumed: whatever they decoded to, the cause is the short scan
    if (fault) atomicOr(&status[sc.image], fault);
}

}  // namespace

extern "C" int maf_jpeg_progressive_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "jpeg_progressive_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_jpeg_scan_t);
    return 0;
}

// The progressive sections of the HOST copy of the blob (maf_jpeg_decode has validated the header's other sections and the image table).
int maf_jpeg_progressive_validate(const uint8_t* hb, const maf_jpeg_header_t& hd) {
    const int64_t T = hd.total_bytes;
    MAF_REQUIRE(hd.n_scans > 0 && hd.n_slanes > 0 && hd.n_rounds > 0 && hd.n_rounds <= hd.n_scans, "jpeg_decode: progressive scans need lanes and rounds");
    MAF_REQUIRE(hd.sgroup >= 1 && hd.sgroup <= MAF_JPEG_GROUP && hd.n_slanes % hd.sgroup == 0, "jpeg_decode: the scan lanes come in whole groups of 1 to MAF_JPEG_GROUP");
    MAF_REQUIRE(in_blob(hd.scans_off, (int64_t)hd.n_scans * (int64_t)sizeof(maf_jpeg_scan_t), T) &&
                in_blob(hd.slanes_off, (int64_t)hd.n_slanes * (int64_t)sizeof(maf_jpeg_lane_t), T) &&
                in_blob(hd.rounds_off, ((int64_t)hd.n_rounds + 1) * 4, T), "jpeg_decode: a progressive blob section lies outside the blob");
    const maf_jpeg_image_t* ims = reinterpret_cast<const maf_jpeg_image_t*>(hb + hd.images_off);
    const maf_jpeg_scan_t* scs = reinterpret_cast<const maf_jpeg_scan_t*>(hb + hd.scans_off);
    const maf_jpeg_lane_t* lns = reinterpret_cast<const maf_jpeg_lane_t*>(hb + hd.slanes_off);
    const int32_t* rounds = reinterpret_cast<const int32_t*>(hb + hd.rounds_off);
    for (int i = 0; i < hd.n_scans; ++i) {
        const maf_jpeg_scan_t& s = scs[i];
        MAF_REQUIRE(s.image >= 0 && s.image < hd.n_images && s.round >= 0 && s.round < hd.n_rounds, "jpeg_decode: a scan's image or round is out of range");
        // rows sorted by image, then round: no two scans of one image share a round (they would race on its coefficients)
        MAF_REQUIRE(i == 0 || s.image > scs[i - 1].image || (s.image == scs[i - 1].image && s.round > scs[i - 1].round),
                    "jpeg_decode: the scan table is not sorted by image and round");
        const maf_jpeg_image_t& m = ims[s.image];
        MAF_REQUIRE(s.ncomp == 1 || (s.ncomp == m.ncomp && s.comp[0] == 0 && s.comp[1] == 1 && s.comp[2] == 2),
                    "jpeg_decode: a scan holds one component or all of them in frame order");
        MAF_REQUIRE(s.comp[0] >= 0 && s.comp[0] < m.ncomp, "jpeg_decode: a scan's component index is out of range");
        MAF_REQUIRE(s.ss >= 0 && s.se <= 63 && s.ss <= s.se && (s.ss != 0 || s.se == 0) && (s.ss == 0 || s.ncomp == 1), "jpeg_decode: bad spectral selection");
        MAF_REQUIRE(s.al >= 0 && s.al <= 13 && (s.ah == 0 || s.ah == s.al + 1), "jpeg_decode: bad successive approximation");
        for (int c = 0; c < 3; ++c) MAF_REQUIRE(s.dc_tab[c] == 0 || s.dc_tab[c] == 1, "jpeg_decode: Huffman table selector out of range");
        MAF_REQUIRE(s.ac_tab == 0 || s.ac_tab == 1, "jpeg_decode: Huffman table selector out of range");
        int bw = m.mcux, bh = m.mcuy;                        // the interleaved grid; a one-component scan: ceil(own samples / 8)
        if (s.ncomp == 1) {
            const int ch = s.comp[0] == 0 ? m.hs : 1, cv = s.comp[0] == 0 ? m.vs : 1;
            const int cw = (m.w * ch + m.hs - 1) / m.hs, chh = (m.h * cv + m.vs - 1) / m.vs;
            bw = (cw + 7) / 8;
            bh = (chh + 7) / 8;
        }
        MAF_REQUIRE(s.bw == bw && s.bh == bh, "jpeg_decode: a scan's MCU grid does not match its image");
    }
    MAF_REQUIRE(rounds[0] == 0 && rounds[hd.n_rounds] == hd.n_slanes, "jpeg_decode: the rounds do not cover the scan lanes");
    const int64_t scan_data = hd.scan_bytes - MAF_JPEG_SCAN_PAD;
    for (int r = 0; r < hd.n_rounds; ++r) {
        MAF_REQUIRE(rounds[r] <= rounds[r + 1] && rounds[r] % hd.sgroup == 0 && rounds[r + 1] <= hd.n_slanes, "jpeg_decode: a round's lanes are not whole groups in order");
        for (int i = rounds[r]; i < rounds[r + 1]; ++i) {
            const maf_jpeg_lane_t& l = lns[i];
            MAF_REQUIRE(l.tabset >= 0 && l.tabset < hd.n_tabsets && l.tabset == lns[i - i % hd.sgroup].tabset, "jpeg_decode: the lanes of a group share one table set");
            if (l.image < 0) continue;
            MAF_REQUIRE(l.image < hd.n_scans && scs[l.image].round == r, "jpeg_decode: a scan lane's scan is out of range or of another round");
            MAF_REQUIRE(l.begin >= 0 && l.begin <= l.end && l.end <= scan_data, "jpeg_decode: a lane's bytes lie outside the scan buffer");
            MAF_REQUIRE(l.first_mcu >= 0 && l.n_mcu >= 0 && (int64_t)l.first_mcu + l.n_mcu <= (int64_t)scs[l.image].bw * scs[l.image].bh,
                        "jpeg_decode: a lane's MCUs lie outside its scan");
        }
    }
    return 0;
}

// One launch per round, in order on the stream (the blob is validated).
int maf_jpeg_progressive_launch(const uint8_t* hb, const uint8_t* db, const maf_jpeg_header_t& hd, int16_t* coef, int32_t* status, hipStream_t s) {
    const int32_t* rounds = reinterpret_cast<const int32_t*>(hb + hd.rounds_off);
    for (int r = 0; r < hd.n_rounds; ++r) {
        const int n = rounds[r + 1] - rounds[r];
        if (n == 0) continue;
        hipLaunchKernelGGL(jpeg_prog_entropy_kernel, dim3(n / hd.sgroup), dim3(MAF_JPEG_GROUP), 0, s,
                           reinterpret_cast<const maf_jpeg_image_t*>(db + hd.images_off), reinterpret_cast<const maf_jpeg_scan_t*>(db + hd.scans_off),
                           reinterpret_cast<const maf_jpeg_lane_t*>(db + hd.slanes_off) + rounds[r], db + hd.huff_off, db + hd.scan_off, hd.scan_bytes,
                           hd.sgroup, coef, status);
        MAF_LAUNCH_CHECK("jpeg_prog_entropy");
    }
    return 0;
}
