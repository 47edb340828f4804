// The multiply-accumulate of the depth-wise conv kernels that work on 16-byte channel vectors (dwconv.hip, dw_branches.hip).
#pragma once
#include "maf_common.h"

// acc[j] += v[j] * w[j] over one 16-byte vector, fp32 accumulate.  For f16 this is v_fma_mix_f32 (f16 sources read
// straight from the packed registers, no v_cvt and no fp32 copies => ~100 fewer VGPRs than cvt + v_pk_fma_f32).
__device__ __forceinline__ void vmac(float (&acc)[8], const half8_t& v, const half8_t& w) {
    const u32x4_t a = __builtin_bit_cast(u32x4_t, v), b = __builtin_bit_cast(u32x4_t, w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[0,0,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * q]) : "v"(a[q]), "v"(b[q]));
        asm("v_fma_mix_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,1,0]" : "+v"(acc[2 * q + 1]) : "v"(a[q]), "v"(b[q]));
    }
}
__device__ __forceinline__ void vmac(float (&acc)[4], const f32x4_t& v, const f32x4_t& w) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(v[j], w[j], acc[j]);
}
