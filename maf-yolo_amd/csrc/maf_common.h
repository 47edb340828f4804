// Shared device/host helpers for libmafyolo_hip (gfx950 only: wave64, MFMA 16x16x32 f16 / 16x16x4 f32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <type_traits>
#include "../../include/mafyolo_hip.h"

typedef _Float16 half_t;
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_t __attribute__((ext_vector_type(2)));

void maf_set_error(const std::string& msg);
int maf_check_hip(hipError_t e, const char* what);

#define MAF_REQUIRE(cond, msg)                          \
    do {                                                \
        if (!(cond)) {                                  \
            maf_set_error(std::string(msg));            \
            return MAF_E_ARG;                           \
        }                                               \
    } while (0)

// behind a kernel launch: a launch error of kernel `name` is recorded and returned
#define MAF_LAUNCH_CHECK(name)                                              \
    do {                                                                    \
        const int rc_ = maf_check_hip(hipGetLastError(), name " launch");   \
        if (rc_) return rc_;                                                \
    } while (0)

// ---- per-kind launchers (each in its own .hip file) ----
int maf_launch_conv_mfma(const maf_op_t* op, hipStream_t s);   // CONV1X1, CONV3X3S2
int maf_launch_stem(const maf_op_t* op, hipStream_t s);
int maf_launch_dwconv(const maf_op_t* op, hipStream_t s);
int maf_launch_sppf_pool(const maf_op_t* op, hipStream_t s);
int maf_launch_decode(const maf_op_t* op, hipStream_t s);
int maf_launch_bottleneck(const maf_op_t* op, hipStream_t s);
int maf_launch_conv1dw(const maf_op_t* op, hipStream_t s);
int maf_launch_head_tail(const maf_op_t* op, hipStream_t s);
int maf_launch_stem2(const maf_op_t* op, hipStream_t s);
int maf_launch_conv3s2_lds(const maf_op_t* op, hipStream_t s);
int maf_launch_conv3s2_wreg(const maf_op_t* op, hipStream_t s);
// depth-wise weight gradient on the matrix cores (dw_wgrad_mfma.hip); MAF_E_UNSUPPORTED = shape not covered, nothing launched
int maf_dw_wgrad_mfma(const void* x, int x_stride, const void* dy, int dy_stride, int B, int H, int W, int C, int k, float* dw, int replicas, hipStream_t s);

// ---- device helpers ----
__device__ __forceinline__ uint8_t clamp_u8(int v) { return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

template <int ACT>
__device__ __forceinline__ float maf_act(float x) {
    if (ACT == MAF_ACT_RELU) return x > 0.f ? x : 0.f;
    if (ACT == MAF_ACT_SILU) return x * __builtin_amdgcn_rcpf(1.f + __expf(-x));      // v_exp + v_rcp (1 ulp), no IEEE divide
    if (ACT == MAF_ACT_SIGMOID) return __builtin_amdgcn_rcpf(1.f + __expf(-x));
    return x;
}
__device__ __forceinline__ float maf_act_rt(float x, int act) {
    switch (act) {
        case MAF_ACT_RELU: return x > 0.f ? x : 0.f;
        case MAF_ACT_SILU: return x * __builtin_amdgcn_rcpf(1.f + __expf(-x));
        case MAF_ACT_SIGMOID: return __builtin_amdgcn_rcpf(1.f + __expf(-x));
        default: return x;
    }
}

// f(std::integral_constant<int, 0>{}) ... f(std::integral_constant<int, N - 1>{}): a loop whose index is a constant expression in the body
// (template arguments, `if constexpr`, asm "n" operands), unrolled by construction
template <int N, int I = 0, typename F>
__device__ __forceinline__ void maf_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        maf_static_for<N, I + 1>(f);
    }
}

// Workgroups go to the 8 XCDs round-robin by block id (block b runs on XCD b % 8), and neighbouring tiles share lines (halos, the channel
// blocks of one tile) that should be fetched into ONE XCD's L2.  Both helpers make the logical tile ids of an XCD contiguous.
//
// One tile per workgroup: the bijective map block id -> logical id of a grid of nwg blocks (the first nwg % 8 XCDs own one id more).
__device__ __forceinline__ int maf_xcd_contiguous_id(int nwg) {
    const int bid = blockIdx.x, xcd = bid & 7, j = bid >> 3;
    const int q = nwg >> 3, r = nwg & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + j;
}
// Persistent workgroups: workgroup wg of nwg walks `for (t = first; t < end; t += step)`, a contiguous eighth of the tiles shared with the
// other workgroups of its XCD.  Needs nwg % 8 == 0 (wg & 7 is then the XCD); otherwise, or with contiguous = false, plain round-robin.
struct maf_tile_walk_t { int first, end, step; };
template <typename I>
__device__ __forceinline__ maf_tile_walk_t maf_xcd_contiguous_walk(I wg, I nwg, int ntiles, bool contiguous = true) {
    maf_tile_walk_t w = {(int)wg, ntiles, (int)nwg};
    if ((nwg & 7) == 0 && contiguous) {
        const int xcd = wg & 7, q = ntiles >> 3, r = ntiles & 7, base = xcd * q + min(xcd, r);
        w.first = base + (int)(wg >> 3); w.end = base + q + (xcd < r ? 1 : 0); w.step = nwg >> 3;
    }
    return w;
}

static inline int maf_cdiv(int a, int b) { return (a + b - 1) / b; }
