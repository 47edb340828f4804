// OpenCV's uint8 INTER_AREA shrink on the device: TrainValDataset.load_image's cv2.resize of an evaluation frame whose longest side exceeds
// the load size (yolov6/data/datasets.py:277-300, r < 1), n frames in one launch.
//
// Pixel rule: tests/area_ref.py (its docstring lists every rule); the kernel equals that restatement bit for bit.  Three paths, chosen on
// the host per frame (maf-yolo_amd/letterbox.py area_plan) and uniform per workgroup:
//   MAF_AREA_FAST2    exact 2 x 2:            (a + b + c + d + 2) >> 2
//   MAF_AREA_FASTN    exact integer factors:  the integer sum of the iscale_y x iscale_x block, float(sum) * inv_area, round half to even
//   MAF_AREA_GENERAL  decimation tables:      per source row of the pixel's y-entries buf = buf + float(S[sx]) * alpha over its x-entries
//                                             (buf starts at 0), sum = beta * buf for the first row, sum = sum + beta * buf after it;
//                                             round half to even, clamp to 0..255.  Every multiply and add is rounded on its own: this
//                                             file is compiled with -ffp-contract=off (an FMA moves results that sit on a rounding tie).
// The tables (start[n_dst + 1] and (source index, alpha) pairs per axis) are built on the host in double; the device does unfused float
// multiplies and adds plus __float2int_rn, no division and no table arithmetic.
//
// Shape.  Grid (bands of AR_ROWS output rows, frames), one output pixel (3 channels) per lane and step, adjacent lanes on adjacent columns,
// plain byte loads: the lanes of a wave read contiguous runs of a few source rows, so each 128-byte line is fetched from HBM once and the
// re-reads of a pixel's other taps hit L1 / L2.  Every destination byte is written exactly once; every source read is inside
// [row * pitch, row * pitch + 3 w) of a row < h (maf_resize_area checks the factors and every table index on the host copy).
#include "maf_common.h"

#include <vector>

namespace {

constexpr int AR_ROWS = 4;                 // output rows per workgroup
constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void resize_area_kernel(const maf_area_frame_t* __restrict__ frames, const int32_t* __restrict__ tab) {
    const maf_area_frame_t f = frames[blockIdx.y];
    const int y0 = blockIdx.x * AR_ROWS;
    if (y0 >= f.new_h) return;                                  // the grid covers the tallest frame
    const int y1 = min(y0 + AR_ROWS, f.new_h);
    const int nw = f.new_w;
    const int n = (y1 - y0) * nw;
    if (f.path == MAF_AREA_FAST2) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int yy = i / nw, x = i - yy * nw, y = y0 + yy;
            const uint8_t* s0 = f.src + (size_t)(2 * y) * f.src_pitch + 6 * x;
            const uint8_t* s1 = s0 + f.src_pitch;
            uint8_t* d = f.dst + ((size_t)y * nw + x) * 3;
            for (int c = 0; c < 3; ++c) d[c] = (uint8_t)(((int)s0[c] + s0[c + 3] + s1[c] + s1[c + 3] + 2) >> 2);
        }
    } else if (f.path == MAF_AREA_FASTN) {
        const int kx = f.iscale_x, ky = f.iscale_y;
        const float inv = f.inv_area;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int yy = i / nw, x = i - yy * nw, y = y0 + yy;
            const uint8_t* s = f.src + (size_t)(ky * y) * f.src_pitch + (size_t)3 * kx * x;
            int a0 = 0, a1 = 0, a2 = 0;
            for (int r = 0; r < ky; ++r, s += f.src_pitch)
                for (int k = 0; k < kx; ++k) { a0 += s[3 * k]; a1 += s[3 * k + 1]; a2 += s[3 * k + 2]; }
            uint8_t* d = f.dst + ((size_t)y * nw + x) * 3;
            d[0] = clamp_u8(__float2int_rn((float)a0 * inv));
            d[1] = clamp_u8(__float2int_rn((float)a1 * inv));
            d[2] = clamp_u8(__float2int_rn((float)a2 * inv));
        }
    } else {
        const int32_t* xs = tab + f.x_start;
        const int32_t* ys = tab + f.y_start;
        const int2* xp = reinterpret_cast<const int2*>(tab + f.x_pairs);       // (source index, alpha bits); the offsets are even
        const int2* yp = reinterpret_cast<const int2*>(tab + f.y_pairs);
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int yy = i / nw, x = i - yy * nw, y = y0 + yy;
            const int kx0 = xs[x], kx1 = xs[x + 1], ky0 = ys[y], ky1 = ys[y + 1];
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int j = ky0; j < ky1; ++j) {
                const int2 ye = yp[j];
                const float beta = __int_as_float(ye.y);
                const uint8_t* row = f.src + (size_t)ye.x * f.src_pitch;
                float b0 = 0.f, b1 = 0.f, b2 = 0.f;
                for (int k = kx0; k < kx1; ++k) {
                    const int2 xe = xp[k];
                    const float alpha = __int_as_float(xe.y);
                    const uint8_t* p = row + 3 * xe.x;
                    b0 = b0 + (float)p[0] * alpha;
                    b1 = b1 + (float)p[1] * alpha;
                    b2 = b2 + (float)p[2] * alpha;
                }
                if (j == ky0) { s0 = beta * b0; s1 = beta * b1; s2 = beta * b2; }
                else { s0 = s0 + beta * b0; s1 = s1 + beta * b1; s2 = s2 + beta * b2; }
            }
            uint8_t* d = f.dst + ((size_t)y * nw + x) * 3;
            d[0] = clamp_u8(__float2int_rn(s0));
            d[1] = clamp_u8(__float2int_rn(s1));
            d[2] = clamp_u8(__float2int_rn(s2));
        }
    }
}

// one axis of a general-path frame on the HOST copy of the tables: start[n_dst + 1] rises from 0, every destination index owns at least one
// entry, all entries lie inside the blob and name a source index below n_src
bool axis_ok(const int32_t* tab, int64_t words, int32_t start, int32_t pairs, int n_src, int n_dst) {
    if (start < 0 || pairs < 0 || (pairs & 1) || (int64_t)start + n_dst + 1 > words) return false;
    const int32_t* s = tab + start;
    if (s[0] != 0) return false;
    for (int i = 0; i < n_dst; ++i)
        if (s[i + 1] <= s[i]) return false;
    const int64_t k = s[n_dst];
    if ((int64_t)pairs + 2 * k > words) return false;
    for (int64_t j = 0; j < k; ++j) {
        const int32_t si = tab[pairs + 2 * j];
        if (si < 0 || si >= n_src) return false;
    }
    return true;
}

struct AxisKey { int32_t start, pairs, n_src, n_dst; };

}  // namespace

extern "C" int maf_area_struct_sizes(int32_t* out) {
    MAF_REQUIRE(out, "area_struct_sizes: null pointer");
    out[0] = (int32_t)sizeof(maf_area_frame_t);
    return 0;
}

extern "C" int maf_resize_area(const maf_area_frame_t* frames, const maf_area_frame_t* frames_dev, int32_t n, const void* tables,
                               const void* tables_dev, int64_t table_words, maf_stream_t stream) {
    MAF_REQUIRE(frames && frames_dev, "resize_area: null pointer (host table and its device copy)");
    MAF_REQUIRE(n > 0 && n <= 65535, "resize_area: n must be positive (at most 65535 frames per launch)");
    MAF_REQUIRE(table_words >= 0 && table_words < ((int64_t)1 << 31), "resize_area: bad table size");
    const int32_t* tab = static_cast<const int32_t*>(tables);
    std::vector<AxisKey> seen;                                   // frames of one size share their tables: each axis is walked once
    auto axis = [&](int32_t start, int32_t pairs, int n_src, int n_dst) {
        for (const AxisKey& k : seen)
            if (k.start == start && k.pairs == pairs && k.n_src == n_src && k.n_dst == n_dst) return true;
        if (!axis_ok(tab, table_words, start, pairs, n_src, n_dst)) return false;
        seen.push_back({start, pairs, n_src, n_dst});
        return true;
    };
    int max_h = 1;
    for (int i = 0; i < n; ++i) {
        const maf_area_frame_t& f = frames[i];
        MAF_REQUIRE(f.src && f.dst, "resize_area: null frame pointer");
        MAF_REQUIRE(f.h > 0 && f.w > 0 && f.new_h > 0 && f.new_w > 0, "resize_area: sizes must be positive");
        MAF_REQUIRE(f.new_w <= f.w && f.new_h <= f.h, "resize_area: new_w / new_h exceed the source (INTER_AREA shrinks; an axis that grows is not supported)");
        MAF_REQUIRE(f.src_pitch >= 3 * (int64_t)f.w, "resize_area: the source row pitch must be at least 3 w bytes");
        MAF_REQUIRE((int64_t)f.new_w * f.new_h < (int64_t)1 << 28 && (int64_t)f.h * f.src_pitch < (int64_t)1 << 40, "resize_area: frame too large");
        if (f.path == MAF_AREA_FAST2 || f.path == MAF_AREA_FASTN) {
            MAF_REQUIRE(f.iscale_x > 0 && f.iscale_y > 0 && (int64_t)f.iscale_x * f.new_w == f.w && (int64_t)f.iscale_y * f.new_h == f.h,
                        "resize_area: a fast-path frame needs exact integer factors (w = iscale_x new_w, h = iscale_y new_h)");
            MAF_REQUIRE(f.path == MAF_AREA_FASTN || (f.iscale_x == 2 && f.iscale_y == 2), "resize_area: the 2 x 2 path needs both factors 2");
        } else {
            MAF_REQUIRE(f.path == MAF_AREA_GENERAL, "resize_area: unknown path");
            MAF_REQUIRE(tables && tables_dev, "resize_area: a general-path frame needs the decimation tables (host copy and device copy)");
            MAF_REQUIRE(axis(f.x_start, f.x_pairs, f.w, f.new_w) && axis(f.y_start, f.y_pairs, f.h, f.new_h),
                        "resize_area: a decimation table is outside the blob, not rising from 0, or names a source index outside the frame");
        }
        max_h = f.new_h > max_h ? f.new_h : max_h;
    }
    hipLaunchKernelGGL(resize_area_kernel, dim3((max_h + AR_ROWS - 1) / AR_ROWS, n), dim3(THREADS), 0, static_cast<hipStream_t>(stream), frames_dev,
                       static_cast<const int32_t*>(tables_dev));
    MAF_LAUNCH_CHECK("resize_area");
    return 0;
}
