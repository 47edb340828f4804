// Block-wide Hillis-Steele scans of one value per thread over a shared array of NT elements, for blocks of NT threads; every thread
// of the block must call.  The array is free again on return.
#pragma once
#include "maf_common.h"

// exclusive prefix sum: the sum of the values of the threads before this one.  T needs T{} (the zero), += and -.
template <int NT, typename T>
__device__ T block_excl_sum(T v, T* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const T t = tid >= d ? sh[tid - d] : T{};
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const T r = sh[tid] - v;
    __syncthreads();
    return r;
}

// inclusive max over the threads after this one (0 when none)
template <int NT>
__device__ double block_suffix_max_after(double v, double* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < NT; d <<= 1) {
        const double t = tid + d < NT ? sh[tid + d] : 0.0;
        __syncthreads();
        sh[tid] = fmax(sh[tid], t);
        __syncthreads();
    }
    const double r = tid + 1 < NT ? sh[tid + 1] : 0.0;
    __syncthreads();
    return r;
}
