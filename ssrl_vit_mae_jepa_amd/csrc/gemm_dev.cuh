// Device helpers shared by the MFMA GEMM files (k_gemm_nt1.hip, k_gemm_nt2.hip, k_gemm_nt3.hip, k_gemm_tn.hip): the block
// remap, the counted wait, the transposed LDS read, the LDS-DMA issue forms, the value pieces of the NT epilogues and the one
// value step that nt1 and nt2 build from them (epi_values8).
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

// ---- pieces of the NT epilogues (k_gemm_nt1 / nt2 / nt3.hip).  The store forms are NOT here: they differ per kernel on purpose
// (nt1 plain, nt2 non-temporal, nt3 buffer stores with a per-piece cache policy), each measured.  nt3 keeps its own mode switch
// over the same pieces (three modes; its register allocation is as sensitive as the note on MAE_REGROUP8 says).

// 8 consecutive outputs of one row as two f32x4: load (fp32 / bf16 side inputs), unpack and pack
__device__ __forceinline__ void unpack8(const bf16x8& v, f32x4& a, f32x4& b) {
  a = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
  b = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
}
__device__ __forceinline__ void ld8(const float* p, f32x4& a, f32x4& b) { a = load4(p); b = load4(p + 4); }
__device__ __forceinline__ void ld8(const bf16* p, f32x4& a, f32x4& b) { unpack8(*reinterpret_cast<const bf16x8*>(p), a, b); }
__device__ __forceinline__ bf16x8 pk8(const f32x4& a, const f32x4& b) {
  return bf16x8{(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
}
// the 16 bytes of the lane 8 places away inside its 16-lane row (DPP row_ror:8; lanes l and l ^ 8 swap)
__device__ __forceinline__ bf16x8 row_swap8(const bf16x8& v) {
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4_;
  u32x4_ x = __builtin_bit_cast(u32x4_, v);
#pragma unroll
  for (int i = 0; i < 4; ++i) x[i] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)x[i], 0x128, 0xf, 0xf, true);
  return __builtin_bit_cast(bf16x8, x);
}
// v = the pre-activation as stored (rounded through the output type), a = fast GELU of it, g = its slope
template <class TO>
__device__ __forceinline__ void gelu_rounded(f32x4& v0, f32x4& v1, f32x4& a0, f32x4& a1, f32x4& g0, f32x4& g1) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    v0[r] = to_f(from_f<TO>(v0[r]));
    v1[r] = to_f(from_f<TO>(v1[r]));
  }
  gelu_fast_pair(v0, a0, g0);
  gelu_fast_pair(v1, a1, g1);
}
// The value step of nt1's and nt2's epilogues, every mode in both output types.  In: v = a lane's 8 accumulators with the bias added,
// q = the (m, n) side input of RESID / DGELU / MUL, loaded or prefetched by the caller (unread in the other modes).  Out: v = the 8
// values for `out`, w = the 8 for `out2` (GELU and GELU_GRAD only).  Loads, stores and the accumulator zeroing stay with the kernel.
constexpr bool epi_side_input(int mode) { return mode == MAE_EPI_RESID || mode == MAE_EPI_DGELU || mode == MAE_EPI_MUL; }
constexpr bool epi_two_outputs(int mode) { return mode == MAE_EPI_GELU || mode == MAE_EPI_GELU_GRAD; }
template <int MODE, class TO>
__device__ __forceinline__ void epi_values8(f32x4& v0, f32x4& v1, const f32x4& q0, const f32x4& q1, f32x4& w0, f32x4& w1) {
  if constexpr (MODE == MAE_EPI_GELU || MODE == MAE_EPI_GELU_GRAD || MODE == MAE_EPI_GELU_ACT) {
    f32x4 a0, a1, g0, g1;
    gelu_rounded<TO>(v0, v1, a0, a1, g0, g1);
    if (MODE == MAE_EPI_GELU) { w0 = a0; w1 = a1; }
    else if (MODE == MAE_EPI_GELU_GRAD) { v0 = g0; v1 = g1; w0 = a0; w1 = a1; }
    else { v0 = a0; v1 = a1; }
  } else if constexpr (MODE == MAE_EPI_RESID) {
    v0 += q0; v1 += q1;
  } else if constexpr (MODE == MAE_EPI_DGELU) {
    f32x4 a_, g_;
    gelu_fast_pair(q0, a_, g_); v0 *= g_;
    gelu_fast_pair(q1, a_, g_); v1 *= g_;
  } else if constexpr (MODE == MAE_EPI_MUL) {
    v0 *= q0; v1 *= q1;
  }
}

// After the MFMAs lane (fq, fr) holds, per 16x16 tile ni, 4 consecutive columns (4 fq ..) of row fr.  One v_permlane16_swap per
// register pair (tiles 2j, 2j+1; lanes l <-> l+16) regroups that into 8 consecutive columns per lane: 16-byte bf16 stores, and
// the 4 lanes of a row cover 64 contiguous bytes per store.  acc is f32x4[MI][NI].
// A macro, not a function template: taking the accumulator array by reference changed the register allocation of 74 of the 84
// gemm_nt3_kernel instantiations (instruction counts -76 .. +8) and of 64 of the 78 gemm_nt2_kernel ones; expanded in place the
// three kernels compile to the instructions they had with the loop written out (profiles/r07_nt_refactor_isa.txt).
#define MAE_REGROUP8(acc, MI, NI)                                                                                  \
  _Pragma("unroll") for (int mi_ = 0; mi_ < (MI); ++mi_)                                                           \
    _Pragma("unroll") for (int j_ = 0; j_ < (NI) / 2; ++j_)                                                        \
      _Pragma("unroll") for (int r_ = 0; r_ < 4; ++r_) {                                                           \
        const auto sw_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(acc[mi_][2 * j_][r_]), __float_as_uint(acc[mi_][2 * j_ + 1][r_]), false, false); \
        acc[mi_][2 * j_][r_] = __uint_as_float(sw_[0]);                                                            \
        acc[mi_][2 * j_ + 1][r_] = __uint_as_float(sw_[1]);                                                        \
      }

}  // namespace mae
