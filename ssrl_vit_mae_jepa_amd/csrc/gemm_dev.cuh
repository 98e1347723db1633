// Device helpers shared by the MFMA GEMM files (k_gemm_mfma.hip, k_gemm_mfma2.hip, k_gemm_nt3.hip, k_gemm_tn.hip): the block
// remap, the counted wait, the transposed LDS read and the LDS-DMA issue forms.
#pragma once
#include "gemm_mfma.h"

namespace mae {

typedef __attribute__((ext_vector_type(4))) int i32x4;

// bijective XCD remap: blocks b and b+8 share an XCD; give every XCD a contiguous run of tiles
__device__ __forceinline__ int64_t xcd_remap(int64_t bid, int64_t nb) {
  const int64_t q = nb >> 3, r = nb & 7, xcd = bid & 7, loc = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// Counted waits.  They assume that vector-memory operations of a wave retire in issue order (LDS-DMA loads and the
// epilogue's stores share one counter, MI355X_MICROARCH: "loads, stores, atomics and LDS-DMA count together, in issue
// order") and that the count a kernel passes equals the number of such instructions the compiler emitted after the one
// waited for.  -DMAE_DBG_VMCNT0 builds the same kernels with every wait drained to zero: tests/test_gpu_kernels.py
// compares the two builds bit for bit (tools/build_dbg_lib.sh vmcnt0), so a miscounted wait shows up as a difference
// instead of a rare wrong tile.
template <int N>
__device__ __forceinline__ void wait_vm() {
#ifdef MAE_DBG_VMCNT0
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#else
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
#endif
}

__device__ __forceinline__ bf16x4 lds_read_tr(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(p));
}

// LDS-DMA through the builtin, 64-bit source pointer (the compiler counts and waits for these itself)
__device__ __forceinline__ void glds16(const bf16* src, char* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
}
__device__ __forceinline__ void glds4(const float* src, char* dst) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src, (__attribute__((address_space(3))) void*)dst, 4, 0, 0);
}

// LDS-DMA pieces from inline asm (the compiler neither counts nor drains them: every wait is the kernel's own).  M0 is written
// in the statement that uses it.  Raw buffer addressing: byte offset = voff (per lane) + soff (scalar), range-checked against
// the descriptor's num_records (out of range -> zeros, no fault).
__device__ __forceinline__ void dma16(const i32x4& rsrc, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
// the same with the non-temporal cache policy (streamed-once rows: the lines are not kept in L2)
__device__ __forceinline__ void dma16_nt(const i32x4& rsrc, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen nt lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ void dma4(const i32x4& rsrc, uint32_t lds_addr, uint32_t voff, uint32_t soff) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tbuffer_load_dword %1, %2, %3 offen lds" ::"s"(lds_addr), "v"(voff), "s"(rsrc), "s"(soff) : "memory");
}
__device__ __forceinline__ i32x4 make_rsrc(const void* p, uint32_t bytes) {
  const uint64_t a = (uint64_t)(uintptr_t)p;
  return i32x4{(int)(uint32_t)a, (int)(uint32_t)((a >> 32) & 0xffffu), (int)bytes, 0x00020000};
}

}  // namespace mae
