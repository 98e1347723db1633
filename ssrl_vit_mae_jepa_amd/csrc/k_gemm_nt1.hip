// Per-tile bf16 MFMA NT GEMM for gfx950 (v_mfma_f32_16x16x32_bf16, fp32 accumulate), fused epilogues: v1, the path of ragged and
// tiny shapes.
//
//  gemm_nt_kernel   out[M,N] = A[M,K] * W[N,K]^T      Linear forward, and dgrad via the transposed weight copy.
//                   Block tile 128 x (64|128) x 64, 4 waves (2x2), register-staged global->LDS with an XOR
//                   swizzle (conflict-free ds_read_b128 fragments), double-buffered LDS, one barrier per K step.
//                   Operands are passed to the MFMA swapped (W as A-operand) so every lane ends up with 4
//                   consecutive output columns of one row: 8-byte (bf16) / 16-byte (fp32) epilogue stores.
//  The weight gradients (dW = dY^T X) are in k_gemm_tn.hip, the persistent LDS-DMA NT kernels in k_gemm_nt2.hip / k_gemm_nt3.hip.
//
// M here is batch*tokens (72 000 .. 290 000), N/K are 192..1536: every GEMM is short-K and output-bound
// (arithmetic intensity ~ the bf16 ridge), so the epilogue stores and the A-panel L2 reuse matter as much as the
// MFMA schedule.  Blocks are remapped so that one XCD walks the N tiles of the same A panel (L2 reuse).
#include "gemm_dev.cuh"

namespace mae {

__device__ __forceinline__ void store8(float* p, const f32x4& a, const f32x4& b) { store4(p, a); store4(p + 4, b); }
__device__ __forceinline__ void store8(bf16* p, const f32x4& a, const f32x4& b) { *reinterpret_cast<bf16x8*>(p) = pk8(a, b); }

// RG ("ragged"): N and K only have to be multiples of 8 (16-byte rows): the last tile column and the last K-step are
// zero-filled on load (predicated, nothing is read out of bounds) and the stores are guarded by column.  This is the
// MFMA path of the reference's shipped tiny config (D = 144: K = 144 / 576, N = 432 / 144 / 576).
template <int MODE, class TO, int NI, bool RG>
__global__ void __launch_bounds__(256, 2) gemm_nt_kernel(const bf16* __restrict__ A, const bf16* __restrict__ W, int64_t M,
                                                         int N, int K, const float* bias, const void* aux, TO* out, TO* out2,
                                                         int tiles_n) {
  constexpr int BM = 128, BN = 32 * NI, BK = 64;
  constexpr int A_BYTES = BM * BK * 2, B_BYTES = BN * BK * 2;
  constexpr int NB = BN / 32;  // 16-byte chunks of the W tile per thread
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;                    // [2][A_BYTES]
  char* sB = smem + 2 * A_BYTES;      // [2][B_BYTES]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int64_t t = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t m0 = (t / tiles_n) * BM;
  const int n0 = (int)(t % tiles_n) * BN;

  // global -> register staging: chunk c = tid + 256 i -> (row c>>3, 16-byte chunk c&7).  Named scalars, not
  // arrays: hipcc kept uint4 staging arrays in scratch memory here (a vmcnt(0) + scratch round trip per load).
  const int srow = tid >> 3, skc = tid & 7;  // chunk i covers row srow + 32 i
  const bf16 *pa0, *pa1, *pa2, *pa3, *pb0, *pb1, *pb2 = nullptr, *pb3 = nullptr;
  {
    auto arow = [&](int i) { int64_t gm = m0 + srow + 32 * i; return A + (gm < M ? gm : M - 1) * K + skc * 8; };  // clamp: rows past M are loaded, never stored
    pa0 = arow(0); pa1 = arow(1); pa2 = arow(2); pa3 = arow(3);
    pb0 = W + (int64_t)(n0 + srow) * K + skc * 8;
    pb1 = pb0 + 32ll * K;
    if (NB > 2) { pb2 = pb0 + 64ll * K; pb3 = pb0 + 96ll * K; }
  }
  // ragged form: which of this thread's W rows exist (rows past N are zero-filled)
  const bool wok0 = !RG || n0 + srow < N, wok1 = !RG || n0 + srow + 32 < N;
  const bool wok2 = !RG || n0 + srow + 64 < N, wok3 = !RG || n0 + srow + 96 < N;
  uint4 ra0, ra1, ra2, ra3, rb0, rb1, rb2 = uint4{0, 0, 0, 0}, rb3 = uint4{0, 0, 0, 0};
  const int soff = srow * 128 + ((skc ^ (srow & 7)) << 4);  // (srow + 32 i) & 7 == srow & 7
  // One 16-byte chunk; ld16p: zero where the ragged form says it does not exist.  The two forms stay two branches: one branch with
  // `ok` a constant true in the plain form cost every plain instantiation a VGPR (profiles/r25_gemm_fallback_refactor_ab.txt).
  auto ld16 = [](const bf16* p, int k0) { return *reinterpret_cast<const uint4*>(p + k0); };
  auto ld16p = [](const bf16* p, int k0, bool ok) { return ok ? *reinterpret_cast<const uint4*>(p + k0) : uint4{0, 0, 0, 0}; };
  auto stage_load = [&](int k0) {
    if (RG) {
      const bool kok = k0 + skc * 8 < K;
      ra0 = ld16p(pa0, k0, kok); ra1 = ld16p(pa1, k0, kok); ra2 = ld16p(pa2, k0, kok); ra3 = ld16p(pa3, k0, kok);
      rb0 = ld16p(pb0, k0, kok && wok0); rb1 = ld16p(pb1, k0, kok && wok1);
      if (NB > 2) { rb2 = ld16p(pb2, k0, kok && wok2); rb3 = ld16p(pb3, k0, kok && wok3); }
    } else {
      ra0 = ld16(pa0, k0); ra1 = ld16(pa1, k0); ra2 = ld16(pa2, k0); ra3 = ld16(pa3, k0);
      rb0 = ld16(pb0, k0); rb1 = ld16(pb1, k0);
      if (NB > 2) { rb2 = ld16(pb2, k0); rb3 = ld16(pb3, k0); }
    }
  };
  auto lds_store = [&](int buf) {
    auto st16 = [&](char* base, int i, const uint4& v) { *reinterpret_cast<uint4*>(base + soff + i * 32 * 128) = v; };
    char* a = sA + buf * A_BYTES;
    char* b = sB + buf * B_BYTES;
    st16(a, 0, ra0); st16(a, 1, ra1); st16(a, 2, ra2); st16(a, 3, ra3);
    st16(b, 0, rb0); st16(b, 1, rb1);
    if (NB > 2) { st16(b, 2, rb2); st16(b, 3, rb3); }
  };

  f32x4 acc[4][NI];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = RG ? (K + BK - 1) / BK : K / BK;
  const int fr = lane & 15, fq = lane >> 4;
  stage_load(0);
  for (int kt = 0; kt < nk; ++kt) {
    const int buf = kt & 1;
    lds_store(buf);
    __syncthreads();
    if (kt + 1 < nk) stage_load((kt + 1) * BK);
    const char* a_base = sA + buf * A_BYTES + (wm * 64 + fr) * 128;
    const char* b_base = sB + buf * B_BYTES + (wn * (NI * 16) + fr) * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int sw = ((ks * 4 + fq) ^ (fr & 7)) << 4;
      bf16x8 af[4], bfr[NI];
#pragma unroll
      for (int mi = 0; mi < 4; ++mi) af[mi] = *reinterpret_cast<const bf16x8*>(a_base + mi * 16 * 128 + sw);
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) bfr[ni] = *reinterpret_cast<const bf16x8*>(b_base + ni * 16 * 128 + sw);
#pragma unroll
      for (int mi = 0; mi < 4; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[ni], af[mi], acc[mi][ni], 0, 0, 0);
    }
  }

  // epilogue: 8 consecutive columns per lane (gemm_dev.cuh)
  MAE_REGROUP8(acc, 4, NI)
  const int gb = (fq & 1) ? 3 + fq : fq;  // 4-column group of this lane inside a 32-column half: {0,4,2,6}[fq]
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
    const int64_t m = m0 + wm * 64 + mi * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < NI / 2; ++j) {
      const int n = n0 + wn * (NI * 16) + 32 * j + 4 * gb;
      if (RG && n >= N) continue;  // N % 8 == 0: a lane's 8 columns are all inside or all outside
      const int64_t o = m * N + n;
      f32x4 v0 = acc[mi][2 * j], v1 = acc[mi][2 * j + 1], q0 = {0.f, 0.f, 0.f, 0.f}, q1 = q0, w0, w1;
      if (bias) { v0 += load4(bias + n); v1 += load4(bias + n + 4); }
      if (epi_side_input(MODE)) ld8(reinterpret_cast<const TO*>(aux) + o, q0, q1);  // RESID's fp32 residual: TO is float there (EpiAll)
      epi_values8<MODE, TO>(v0, v1, q0, q1, w0, w1);
      store8(out + o, v0, v1);
      if (epi_two_outputs(MODE)) store8(out2 + o, w0, w1);
    }
  }
}

template <int MODE, class TO, int NI, bool RG = false>
static int launch_nt(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& e, hipStream_t s) {
  constexpr int BN = 32 * NI;
  const int tiles_n = RG ? (int)cdiv(N, BN) : N / BN;
  const int64_t tiles = cdiv(M, 128) * tiles_n;
  MAE_REQUIRE(tiles < (1ll << 31), "gemm: grid too large");
  const size_t lds = 2 * (128 * 64 * 2) + 2 * (BN * 64 * 2);
  auto kern = gemm_nt_kernel<MODE, TO, NI, RG>;
  MAE_TRY(allow_lds(kern, lds));   // 48 or 64 KiB: inside the default limit
  hipLaunchKernelGGL(kern, dim3((unsigned)tiles), dim3(256), lds, s, A, W, M, N, K, e.bias, e.aux, (TO*)e.out, (TO*)e.out2, tiles_n);
  MAE_LAUNCH_CHECK();
  return 0;
}

template <int MODE, class TO>
static int launch_nt_ni(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& e, hipStream_t s) {
  if (K % 64 != 0 || N % 64 != 0) return launch_nt<MODE, TO, 2, true>(A, W, M, N, K, e, s);  // ragged: 128 x 64 tiles
  if (N % 128 == 0) return launch_nt<MODE, TO, 4>(A, W, M, N, K, e, s);
  return launch_nt<MODE, TO, 2>(A, W, M, N, K, e, s);
}

int mfma_linear_fwd(const bf16* A, const bf16* W, int64_t M, int N, int K, const Epi& e, hipStream_t s) {
  if (K % 8 != 0 || N % 8 != 0 || K < 32 || N < 16 || M < 1) return MFMA_UNSUPPORTED;
  if ((((uintptr_t)A | (uintptr_t)W | (uintptr_t)e.out | (uintptr_t)e.out2 | (uintptr_t)e.aux | (uintptr_t)e.bias) & 15) != 0)
    return MFMA_UNSUPPORTED;
  return dispatch_epi<EpiAll>(e, [&](auto mode, auto to) {
    return launch_nt_ni<decltype(mode)::value, typename decltype(to)::type>(A, W, M, N, K, e, s);
  });
}

}  // namespace mae
