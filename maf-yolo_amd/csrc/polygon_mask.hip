// Polygon masks on the device: the image cv2.drawContours(im_new, [contour], -1, (1, 1, 1), cv2.FILLED) leaves for the contours copy_paste
// picks (yolov6/data/data_augment.py:285-307), one bit per canvas pixel, all masks of a batch in one launch.
//
// Fill rule: tests/copy_paste_ref.py (its docstring states every rule; OpenCV's fillPoly with line_type 8, shift 0, restated); the kernel
// equals that restatement bit for bit.  Per contour the mask is the union of
//   (a) every edge as cv::LineIterator's 8-connected line, after cv::clipLine moved its endpoints into the canvas.  The iterator's pixel k
//       has the closed form major = start + k, minor = start + (2 d k + D - 1) / (2 D) (D, d: major and minor lengths), so a lane that owns
//       an edge visits only the k whose row lies in its workgroup's band;
//   (b) the even-odd scan-line interior: an edge with upper vertex (x0, y0) crosses row y at x = (x0 << 16) + (y - y0) step in 16.16 fixed
//       point, step = ((x1 - x0) << 16) / (y1 - y0) truncated.  OpenCV pairs the sorted crossings of a row and fills (xl + 65535) >> 16 ..
//       xr >> 16; column c is therefore set iff an odd number of crossings lie below c << 16, or one lies exactly on it.  Each crossing
//       toggles ONE bit (column (x >> 16) + 1) of a delta row; a prefix XOR along the row turns the toggles into the parity.
//
// Shape.  Grid (bands of PM_ROWS canvas rows, masks), 256 lanes.  A workgroup holds its band twice in LDS (the mask so far, the toggles of
// the contour in hand): lanes take the edges of one contour (LDS atomics: or for pixels, xor for toggles), then each 32-lane half of a wave
// scans one row (in-word prefix XOR by shifts, the carry across words from a wave ballot of the words' parities) and ors it into the mask;
// contours of one mask follow each other, which keeps their parities apart (the union of contours is an OR, not an XOR).  The band then
// leaves as plain coalesced 32-bit stores: every word of every mask is written exactly once, a mask without contours as zeros.  No global
// atomics; 64-bit integer edge arithmetic, no floating point (clipLine's double quotient equals the truncating integer division for the
// coordinate range the entry admits: tests/copy_paste_ref.py).  All LDS indices are formed from clipped coordinates and checked again
// against the band before use.
#include "maf_common.h"

namespace {

constexpr int PM_ROWS = 8;                 // rows per workgroup: one per 32-lane half-wave in the scan
constexpr int PM_THREADS = 256;
static_assert(PM_THREADS == 32 * PM_ROWS, "the scan gives each row of the band one 32-lane half-wave");

struct pm_line_t { int x1, y1, x2, y2; bool any; };

// cv::clipLine(Size(C, C), p1, p2): Cohen-Sutherland with truncating quotients; any = false when nothing of the segment is inside
__device__ __forceinline__ pm_line_t pm_clip_line(int C, long long x1, long long y1, long long x2, long long y2) {
    const long long right = C - 1, bottom = C - 1;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        if (c1 & 12) {
            const long long a = c1 < 8 ? 0 : bottom;
            x1 += (a - y1) * (x2 - x1) / (y2 - y1);
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            const long long a = c2 < 8 ? 0 : bottom;
            x2 += (a - y2) * (x2 - x1) / (y2 - y1);
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                const long long a = c1 == 1 ? 0 : right;
                y1 += (a - x1) * (y2 - y1) / (x2 - x1);
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                const long long a = c2 == 1 ? 0 : right;
                y2 += (a - x2) * (y2 - y1) / (x2 - x1);
                x2 = a;
                c2 = 0;
            }
        }
    }
    pm_line_t l = {(int)x1, (int)y1, (int)x2, (int)y2, (c1 | c2) == 0};
    return l;
}

__device__ __forceinline__ void pm_set(uint32_t* band, int W, int C, int b0, int b1, int x, int y) {
    if (x >= 0 && x < C && y >= b0 && y < b1) atomicOr(&band[(y - b0) * W + (x >> 5)], 1u << (x & 31));
}

// the first pixel index k of a LineIterator whose minor coordinate has advanced m steps (m_k = (2 d k + D - 1) / (2 D) >= m)
__device__ __forceinline__ long long pm_first_k(long long D, long long d, long long m) {
    if (m <= 0) return 0;
    if (d == 0) return D + 1;                                   // a line along its major axis never steps sideways
    return (2 * D * m - D) / (2 * d) + 1;
}

// (a): the pixels of edge p -> q that fall on rows [b0, b1)
__device__ __forceinline__ void pm_draw_line(uint32_t* band, int W, int C, int b0, int b1, int px, int py, int qx, int qy) {
    const pm_line_t l = pm_clip_line(C, px, py, qx, qy);
    if (!l.any) return;
    int x1 = l.x1, y1 = l.y1, dx = l.x2 - l.x1, dy = l.y2 - l.y1, sy = 1;
    if (dx < 0) { dx = -dx; dy = -dy; x1 = l.x2; y1 = l.y2; }     // leftToRight
    if (dy < 0) { dy = -dy; sy = -1; }
    const bool vert = dy > dx;
    const long long D = vert ? dy : dx, d = vert ? dx : dy;
    long long k0, k1;                                           // the k whose row may lie in the band: [k0, k1]
    if (vert) {
        k0 = sy > 0 ? (long long)b0 - y1 : (long long)y1 - b1 + 1;
        k1 = sy > 0 ? (long long)b1 - 1 - y1 : (long long)y1 - b0;
    } else {
        const long long m0 = sy > 0 ? (long long)b0 - y1 : (long long)y1 - b1 + 1, m1 = sy > 0 ? (long long)b1 - 1 - y1 : (long long)y1 - b0;
        if (m1 < 0) return;
        k0 = pm_first_k(D, d, m0);
        k1 = pm_first_k(D, d, m1 + 1) - 1;
    }
    k0 = k0 < 0 ? 0 : k0;
    k1 = k1 > D ? D : k1;
    for (long long k = k0; k <= k1; ++k) {
        const int t = D > 0 ? (int)((2 * d * k + D - 1) / (2 * D)) : 0;
        const int x = vert ? x1 + t : x1 + (int)k, y = vert ? y1 + sy * (int)k : y1 + sy * t;
        pm_set(band, W, C, b0, b1, x, y);
    }
}

// (b): the crossings of edge p -> q with rows [b0, b1): one toggle each, and the pixel a crossing lands on exactly
__device__ __forceinline__ void pm_cross(uint32_t* band, uint32_t* delta, int W, int C, int b0, int b1, int px, int py, int qx, int qy) {
    if (py == qy) return;
    const long long x0 = py < qy ? px : qx, y0 = py < qy ? py : qy, x1 = py < qy ? qx : px, y1 = py < qy ? qy : py;
    const long long step = (x1 - x0) * 65536 / (y1 - y0);
    const int ya = y0 > b0 ? (int)y0 : b0, yb = y1 < b1 ? (int)y1 : b1;
    for (int y = ya; y < yb; ++y) {
        const long long x = x0 * 65536 + (y - y0) * step;
        const long long c = x >> 16;                            // floor
        if ((x & 0xFFFF) == 0) pm_set(band, W, C, b0, b1, c < 0 ? -1 : (c >= C ? -1 : (int)c), y);
        const int p = c + 1 < 0 ? 0 : (c + 1 > C ? C : (int)(c + 1));
        if (p < C) atomicXor(&delta[(y - b0) * W + (p >> 5)], 1u << (p & 31));
    }
}

// table: mask_start [n + 1] | poly_start [npoly + 1] | xy [2 nvert]
__global__ __launch_bounds__(PM_THREADS) void polygon_mask_kernel(const int32_t* __restrict__ table, int n, int npoly, int C, int W,
                                                                   uint32_t* __restrict__ out) {
    extern __shared__ uint32_t pm_lds[];
    uint32_t* band = pm_lds;                                    // [PM_ROWS][W]: the mask so far
    uint32_t* delta = pm_lds + PM_ROWS * W;                     // [PM_ROWS][W]: the toggles of the contour in hand
    const int tid = threadIdx.x, mask = blockIdx.y;
    const int b0 = blockIdx.x * PM_ROWS, b1 = min(b0 + PM_ROWS, C);
    const int32_t* poly_start = table + n + 1;
    const int32_t* xy = poly_start + npoly + 1;
    for (int i = tid; i < 2 * PM_ROWS * W; i += PM_THREADS) pm_lds[i] = 0u;
    __syncthreads();
    const int row = tid >> 5, lane = tid & 31;
    for (int p = table[mask]; p < table[mask + 1]; ++p) {
        const int v0 = poly_start[p], nv = poly_start[p + 1] - v0;
        for (int e = tid; e < nv; e += PM_THREADS) {
            const int a = v0 + (e == 0 ? nv - 1 : e - 1), b = v0 + e;
            const int px = xy[2 * a], py = xy[2 * a + 1], qx = xy[2 * b], qy = xy[2 * b + 1];
            pm_draw_line(band, W, C, b0, b1, px, py, qx, qy);
            pm_cross(band, delta, W, C, b0, b1, px, py, qx, qy);
        }
        __syncthreads();
        uint32_t carry = 0u;                                    // parity of the toggles in the words before this chunk
        for (int w0 = 0; w0 < W; w0 += 32) {
            const int w = w0 + lane;
            uint32_t v = w < W ? delta[row * W + w] : 0u;
            v ^= v << 1; v ^= v << 2; v ^= v << 4; v ^= v << 8; v ^= v << 16;      // bit i = parity of bits 0..i
            const unsigned long long odd = __ballot(v >> 31);
            const uint32_t half = (uint32_t)(odd >> (tid & 32));                   // this row's 32 lanes
            const uint32_t before = carry ^ (__popc(half & ((1u << lane) - 1u)) & 1u);
            if (w < W) {
                band[row * W + w] |= v ^ (before ? 0xFFFFFFFFu : 0u);
                delta[row * W + w] = 0u;
            }
            carry ^= __popc(half) & 1u;
        }
        __syncthreads();
    }
    const uint32_t tail = (C & 31) ? (1u << (C & 31)) - 1u : 0xFFFFFFFFu;          // the padding bits of a row's last word stay 0
    uint32_t* o = out + ((size_t)mask * C + b0) * W;
    for (int i = tid; i < (b1 - b0) * W; i += PM_THREADS) o[i] = band[i] & ((i % W) == W - 1 ? tail : 0xFFFFFFFFu);
}

}  // namespace

extern "C" int maf_polygon_mask(const int32_t* table, const int32_t* table_dev, int32_t n, int32_t npoly, int32_t nvert, int32_t C, uint32_t* masks,
                                maf_stream_t stream) {
    MAF_REQUIRE(table && table_dev && masks, "polygon_mask: null pointer (host table, its device copy, masks)");
    MAF_REQUIRE((reinterpret_cast<uintptr_t>(masks) & 3) == 0 && (reinterpret_cast<uintptr_t>(table_dev) & 3) == 0, "polygon_mask: masks and table_dev must be 4-byte aligned");
    MAF_REQUIRE(n > 0 && n <= MAF_POLYGON_MAX_MASKS, "polygon_mask: n must be in 1..65535");
    MAF_REQUIRE(C > 0 && C <= MAF_POLYGON_MAX_CANVAS, "polygon_mask: C must be in 1..16384");
    MAF_REQUIRE(npoly >= 0 && nvert >= 0 && npoly <= MAF_POLYGON_MAX_CONTOURS && nvert <= MAF_POLYGON_MAX_VERTICES, "polygon_mask: npoly / nvert out of range");
    const int32_t* mask_start = table;
    const int32_t* poly_start = table + n + 1;
    const int32_t* xy = poly_start + npoly + 1;
    MAF_REQUIRE(mask_start[0] == 0 && mask_start[n] == npoly, "polygon_mask: mask_start must rise from 0 to npoly");
    for (int i = 0; i < n; ++i) MAF_REQUIRE(mask_start[i] <= mask_start[i + 1], "polygon_mask: mask_start must rise from 0 to npoly");
    MAF_REQUIRE(poly_start[0] == 0 && poly_start[npoly] == nvert, "polygon_mask: poly_start must rise strictly from 0 to nvert (a contour has a vertex)");
    for (int i = 0; i < npoly; ++i)
        MAF_REQUIRE(poly_start[i] < poly_start[i + 1], "polygon_mask: poly_start must rise strictly from 0 to nvert (a contour has a vertex)");
    for (int64_t i = 0; i < 2 * (int64_t)nvert; ++i)
        MAF_REQUIRE(xy[i] >= -MAF_POLYGON_COORD_MAX && xy[i] <= MAF_POLYGON_COORD_MAX, "polygon_mask: a vertex coordinate is outside [-32767, 32767]");
    const int W = (C + 31) / 32;
    hipLaunchKernelGGL(polygon_mask_kernel, dim3((C + PM_ROWS - 1) / PM_ROWS, n), dim3(PM_THREADS), 2 * PM_ROWS * W * sizeof(uint32_t),
                       static_cast<hipStream_t>(stream), table_dev, (int)n, (int)npoly, (int)C, W, masks);
    return maf_check_hip(hipGetLastError(), "polygon_mask launch");
}
