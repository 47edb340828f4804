// LDS fragment reads as inline assembly with hand-counted waits, shared by the kernels whose MFMA operands come out of LDS: the one home of
// the reads (lp_ds_read_*), of the waits (lp_wait_lgkm, lp_wait_vm) and of the explanation.
//
// Written as plain loads, hipcc (ROCm 7.2) reads one or two fragments into the same register quads right in front of the MFMAs that need them and
// waits with lgkmcnt(1) / lgkmcnt(0): a full LDS round trip (~130 cycles) per one or two 17-cycle MFMAs (measured: 9.4k of the 9.6k cycles of a
// conv3s2_wreg tile, 4.7k instead of 1.2k for the 72 MFMAs of a 288 -> 128 conv1x1_stream_lds tile).  The pattern used instead: the read of
// step t + RD is issued before the MFMAs of step t; LDS operations return in order, so when step t is consumed at most min(RD, steps left)
// newer reads may still be in flight: `s_waitcnt lgkmcnt(that)`.  (Scalar loads share the counter; one in flight only makes a wait longer.)
//
// The compiler knows nothing of this counting: to it the asm read has written its destination when the statement ends, and nothing would
// keep it from scheduling the MFMA that consumes the registers above the `s_waitcnt`.  Hence lp_wait_lgkm<N>(regs...) takes the registers
// that the wait makes valid as "+v" operands: the wait "rewrites" them, so whatever reads them stays below it.  Pass every register that
// is consumed after this wait and was not covered by an earlier one.  The forms without operands carry a "memory" clobber instead: they
// order plain loads and stores (a DMA into LDS has landed, the compiler's own LDS reads are complete) and pin no register.
#pragma once
#include "maf_common.h"

template <int OFF> __device__ __forceinline__ void lp_ds_read_b128(u32x4_t& d, uint32_t addr) { asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF)); }
template <int OFF> __device__ __forceinline__ void lp_ds_read_b64(u32x2_t& d, uint32_t addr) { asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF)); }

// A, B, C: u32x4_t or u32x2_t, whatever the reads above filled
template <int N, typename A> __device__ __forceinline__ void lp_wait_lgkm(A& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N)); }
template <int N, typename A, typename B> __device__ __forceinline__ void lp_wait_lgkm(A& a, B& b) { asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N)); }
template <int N, typename A, typename B, typename C> __device__ __forceinline__ void lp_wait_lgkm(A& a, B& b, C& c) { asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(a), "+v"(b), "+v"(c) : "n"(N)); }
template <int N> __device__ __forceinline__ void lp_wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }
template <int N> __device__ __forceinline__ void lp_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

__device__ __forceinline__ uint32_t lp_lds_addr(const void* p) { return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p; }
