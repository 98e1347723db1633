// bf16 MFMA GEMM kernels (k_gemm_nt1 / nt2 / nt3.hip, k_gemm_tn.hip, k_attention_mfma.hip): entry points used by the dispatch in
// k_gemm.hip, and the host pieces the three NT files share.  Each entry point returns MFMA_UNSUPPORTED when the shape or the
// epilogue is outside what its kernel takes; the caller then tries the next kernel, and last the generic kernel (launch_generic,
// k_gemm.hip).  The device pieces, the 8-column epilogue value step of v1 and v2 among them, are in gemm_dev.cuh.
#pragma once
#include "kernels.h"
#include <type_traits>

namespace mae {

constexpr int MFMA_UNSUPPORTED = -7777;

// out[M,N] = A[M,K] * W[N,K]^T (+bias) with an Epi epilogue, three kernels:
// v1, gemm_nt_kernel (k_gemm_nt1.hip): per-tile, register-staged.  Every epilogue in both output types (RESID fp32 only);
// K % 8 == 0, N % 8 == 0, K >= 32, N >= 16: the path of ragged and tiny shapes.
int mfma_linear_fwd(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& epi, hipStream_t s);

// v2, gemm_nt2_kernel (k_gemm_nt2.hip): persistent LDS-DMA ring, 64-bit pointers.  The same epilogues as v1; N % 128 == 0 or
// N % 192 == 0, K % 64 == 0, K >= 192.  Serves what v3 leaves (GELU, RESID, DGELU, fp32 GELU_GRAD / GELU_ACT / MUL) and is the
// reference the tests compare v3 with bit for bit.
int mfma_linear_fwd_v2(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& epi, hipStream_t s);

// v3, gemm_nt3_kernel (k_gemm_nt3.hip): the production K-loop on v2's tiles, 32-bit buffer offsets.  NONE in both output types,
// GELU_GRAD / GELU_ACT / MUL with bf16 outputs (what the engine issues); v2's shapes while operands and outputs stay below 4 GiB.
// w2: two 4-wave workgroups per CU on 128-row tiles (MAE_GEMM_NT=v3w2, A/B).
int mfma_linear_fwd_v3(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& epi, bool w2, hipStream_t s);

// The epilogue mode x output type switch of the three entry points above: calls f(EpiMode<MODE>{}, OutType<TO>{}) for e's mode and
// output type when SUP::ok(MODE, fp32 output), the kernel's own compile-time list, has it (nothing else is instantiated), and
// returns MFMA_UNSUPPORTED otherwise.
template <int MODE> using EpiMode = std::integral_constant<int, MODE>;
template <class TO> struct OutType { using type = TO; };
template <class SUP, class F>
int dispatch_epi(const Epi& e, F&& f) {
  auto typed = [&](auto mode) -> int {
    constexpr int MODE = decltype(mode)::value;
    if (e.out_dt == MAE_F32) {
      if constexpr (SUP::ok(MODE, true)) return f(mode, OutType<float>{});
    } else {
      if constexpr (SUP::ok(MODE, false)) return f(mode, OutType<bf16>{});
    }
    return MFMA_UNSUPPORTED;
  };
  switch (e.mode) {
    case MAE_EPI_NONE: return typed(EpiMode<MAE_EPI_NONE>{});
    case MAE_EPI_GELU: return typed(EpiMode<MAE_EPI_GELU>{});
    case MAE_EPI_RESID: return typed(EpiMode<MAE_EPI_RESID>{});
    case MAE_EPI_DGELU: return typed(EpiMode<MAE_EPI_DGELU>{});
    case MAE_EPI_GELU_GRAD: return typed(EpiMode<MAE_EPI_GELU_GRAD>{});
    case MAE_EPI_MUL: return typed(EpiMode<MAE_EPI_MUL>{});
    case MAE_EPI_GELU_ACT: return typed(EpiMode<MAE_EPI_GELU_ACT>{});
    default: return MFMA_UNSUPPORTED;
  }
}
struct EpiAll {   // v1 and v2: every mode; RESID adds an fp32 residual and writes fp32
  static constexpr bool ok(int mode, bool f32out) { return mode != MAE_EPI_RESID || f32out; }
};

// launch of a persistent NT kernel (v2, v3) in its with-bias or its without-bias instantiation
template <class KB, class KN, class... Args>
int launch_bias_pair(bool has_bias, KB with_bias, KN without, int grid, int block, int lds, hipStream_t s, Args... args) {
  auto go = [&](auto kern) -> int {
    MAE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, s, args...);
    MAE_LAUNCH_CHECK();
    return 0;
  };
  return has_bias ? go(with_bias) : go(without);
}

// v2 / v3, widths that are multiples of 192: 192-row tiles instead of 256-row ones?  Rounds of tiles on the CUs x rows per tile is the
// time proxy; the 192-row tile must win by margin_pct (it stages 15 % more operand bytes per flop).  MAE_NT_BM=192|256 forces (A/B).
bool prefer_bm192(int64_t M, int N, int margin_pct);

// weight gradient (k_gemm_tn.hip): dW[N,K] = dY[M,N]^T * A[M,K] (fp32, written)
int64_t mfma_wgrad_scratch_bytes(int64_t M, int N, int K);
// also db[N] = column sums of dY when db != null
int mfma_linear_wgrad(const bf16* dY, const bf16* A, int64_t M, int N, int K, float* dW, float* db, void* slab, hipStream_t s);

// two weight gradients that share M in one launch (one tile list, M-splits chosen for the sum); MFMA_UNSUPPORTED when either
// shape is not one of the 192 x 192 ring kernel's, M < 8192, a bias gradient is missing, or an A/B switch is set
int64_t mfma_wgrad_pair_scratch_bytes(int64_t M, int N0, int K0, int N1, int K1);
int mfma_linear_wgrad_pair(const bf16* dY0, const bf16* A0, int N0, int K0, float* dW0, float* db0, const bf16* dY1, const bf16* A1,
                           int N1, int K1, float* dW1, float* db1, int64_t M, void* slab, hipStream_t s);

// attention (k_attention_mfma.hip)
int mfma_attention_fwd(const bf16* qkv, int B, int T, int H, int hd, bf16* out, float* lse, hipStream_t s);
int mfma_attention_bwd(const bf16* qkv, const bf16* out, const bf16* d_out, const float* lse, int B, int T, int H, int hd,
                       bf16* d_qkv, hipStream_t s);

}  // namespace mae
