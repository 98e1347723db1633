// bf16 MFMA weight-gradient GEMMs for gfx950 (v_mfma_f32_16x16x32_bf16, fp32 accumulate).
//
//   dW[N,K] = dY[M,N]^T * X[M,K],  db[N] = column sums of dY:  the reduction runs over the long M dimension (batch*tokens,
//   72 000 .. 290 000) and is split over M into fp32 slabs that an ordered (deterministic) reduce sums.
//
//  gemm_tn_kernel   register-staged 128 x 128 (or 64-wide) tiles: both operand tiles are [m][*] row-major in LDS and read transposed
//                   with ds_read_b64_tr_b16.  Any N, K that are multiples of 8; MAE_WGRAD=v1 pins it.
//  gemm_tn4_kernel  192 x 192 tiles fed by a three-stage LDS-DMA ring, buffer-descriptor DMA: the default.
//  gemm_tn3_kernel  the same tiles, ring and schedule with 64-bit-pointer DMA: the path for matrices beyond 32-bit byte offsets
//                   and the reference the tests compare tn4 against bit for bit (MAE_WGRAD=v3r).
#include "gemm_dev.cuh"
#include <cstdlib>
#include <cstring>

namespace mae {

constexpr int TN_RS = 288;  // LDS row stride in bytes for a 128-column bf16 tile row (256 B + 32 B pad): consecutive rows
                            // shift by 8 banks, so the 8 rows one 32-lane half reads transposed are conflict-free

// NI / KI: 16-wide tiles per wave along n / k (block tile = 32*NI x 32*KI), reduction step 64 rows of m
// RG ("ragged"): N and K multiples of 8 only; tile columns past N / K are zero-filled on load, stores are guarded.
template <int NI, int KI, bool RG>
__global__ void __launch_bounds__(256, 2) gemm_tn_kernel(const bf16* __restrict__ dY, const bf16* __restrict__ X, int64_t M, int N,
                                                         int K, float* __restrict__ out, float* __restrict__ db,
                                                         int64_t split_stride, int tiles_n, int tiles_k, int64_t m_chunk) {
  constexpr int TNB = 32 * NI, TKB = 32 * KI, BR = 64;
  constexpr int Y_BYTES = BR * TN_RS, X_BYTES = BR * TN_RS;
  constexpr int YC = TNB / 8 * BR / 256;  // 16-byte chunks per thread for the dY tile (TNB/8 chunks per row)
  constexpr int XC = TKB / 8 * BR / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sY = smem;                 // [2][Y_BYTES]
  char* sX = smem + 2 * Y_BYTES;   // [2][X_BYTES]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave >> 1, wk = wave & 1;
  // XCD-aware order: every tile of one M-chunk ("split") runs on the same XCD at the same time, so the chunk's dY and X
  // rows are fetched from HBM once and shared through that XCD's L2 (round-robin placement re-fetched them per XCD:
  // 908 MB of HBM reads per launch against 221 MB of operands, rocprofv3 FETCH_SIZE)
  const int vb = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int tile = vb % (tiles_n * tiles_k);
  const int split = vb / (tiles_n * tiles_k);
  const int n0 = (tile / tiles_k) * TNB, k0 = (tile % tiles_k) * TKB;
  const int64_t mbeg = (int64_t)split * m_chunk;
  const int64_t mend = mbeg + m_chunk < M ? mbeg + m_chunk : M;

  uint4 ry[YC], rx[XC];
#define TN_G_LOAD(mb)                                                                         \
  {                                                                                           \
    _Pragma("unroll") for (int i = 0; i < YC; ++i) {                                          \
      const int c = tid + 256 * i, row = c / (TNB / 8), cc = c % (TNB / 8);                   \
      const int64_t m = (mb) + row;                                                           \
      ry[i] = (m < mend && (!RG || n0 + cc * 8 < N)) ? *reinterpret_cast<const uint4*>(dY + m * N + n0 + cc * 8) : uint4{0, 0, 0, 0}; \
    }                                                                                         \
    _Pragma("unroll") for (int i = 0; i < XC; ++i) {                                          \
      const int c = tid + 256 * i, row = c / (TKB / 8), cc = c % (TKB / 8);                   \
      const int64_t m = (mb) + row;                                                           \
      rx[i] = (m < mend && (!RG || k0 + cc * 8 < K)) ? *reinterpret_cast<const uint4*>(X + m * K + k0 + cc * 8) : uint4{0, 0, 0, 0}; \
    }                                                                                         \
  }
#define TN_S_STORE(buf)                                                                       \
  {                                                                                           \
    _Pragma("unroll") for (int i = 0; i < YC; ++i) {                                          \
      const int c = tid + 256 * i, row = c / (TNB / 8), cc = c % (TNB / 8);                   \
      *reinterpret_cast<uint4*>(sY + (buf) * Y_BYTES + row * TN_RS + cc * 16) = ry[i];        \
    }                                                                                         \
    _Pragma("unroll") for (int i = 0; i < XC; ++i) {                                          \
      const int c = tid + 256 * i, row = c / (TKB / 8), cc = c % (TKB / 8);                   \
      *reinterpret_cast<uint4*>(sX + (buf) * X_BYTES + row * TN_RS + cc * 16) = rx[i];        \
    }                                                                                         \
  }

  f32x4 acc[KI][NI], accb[NI];
#pragma unroll
  for (int i = 0; i < KI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < NI; ++j) accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias gradient = column sums of dY: one extra MFMA per n-tile against an all-ones operand, done by the waves
  // that own the first k tile (wave-uniform condition)
  const bool do_bias = db != nullptr && k0 == 0 && wk == 0;
  const bf16 one = (bf16)1.0f;
  const bf16x8 ones = bf16x8{one, one, one, one, one, one, one, one};

  // transposed-read address of this lane inside a 32-row k-substep: rows 16h + 4g + q, columns cb + 4p .. 4p+3
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int lane_off = (4 * g + q) * TN_RS + p * 8;

  const int64_t nsteps = (mend - mbeg + BR - 1) / BR;
#ifndef MAE_DBG_TN_NO_LOAD
  TN_G_LOAD(mbeg)
#else
  for (int i = 0; i < YC; ++i) ry[i] = uint4{0, 0, 0, 0};
  for (int i = 0; i < XC; ++i) rx[i] = uint4{0, 0, 0, 0};
#endif
  for (int64_t st = 0; st < nsteps; ++st) {
    const int buf = (int)(st & 1);
    TN_S_STORE(buf)
    __syncthreads();
#ifndef MAE_DBG_TN_NO_LOAD
    if (st + 1 < nsteps) TN_G_LOAD(mbeg + (st + 1) * BR)
#endif
#ifdef MAE_DBG_TN_NO_MFMA
    continue;
#endif
    const char* yb = sY + buf * Y_BYTES + lane_off + (wn * NI * 16) * 2;
    const char* xb = sX + buf * X_BYTES + lane_off + (wk * KI * 16) * 2;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 yf[NI], xf[KI];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const bf16x4 lo = lds_read_tr(yb + (ks * 32) * TN_RS + ni * 32);
        const bf16x4 hi = lds_read_tr(yb + (ks * 32 + 16) * TN_RS + ni * 32);
        yf[ni] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int ki = 0; ki < KI; ++ki) {
        const bf16x4 lo = lds_read_tr(xb + (ks * 32) * TN_RS + ki * 32);
        const bf16x4 hi = lds_read_tr(xb + (ks * 32 + 16) * TN_RS + ki * 32);
        xf[ki] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      }
#pragma unroll
      for (int ki = 0; ki < KI; ++ki)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
          acc[ki][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf[ki], yf[ni], acc[ki][ni], 0, 0, 0);
      if (do_bias) {
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) accb[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, yf[ni], accb[ni], 0, 0, 0);
      }
    }
  }
  // D[i = k][j = n]: lane holds n = tile col (lane&15), k = 4*(lane>>4) + r -> 16-byte store along k
  float* o = out + (int64_t)split * split_stride;
  if (do_bias && lane < 16) {  // every row of the ones-product is the same column sum: take row 0
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
      const int n = n0 + wn * NI * 16 + ni * 16 + lane;
      if (!RG || n < N) db[(int64_t)split * split_stride + n] = accb[ni][0];
    }
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int n = n0 + wn * NI * 16 + ni * 16 + (lane & 15);
#pragma unroll
    for (int ki = 0; ki < KI; ++ki) {
      const int k = k0 + wk * KI * 16 + ki * 16 + (lane >> 4) * 4;
      if (!RG || (n < N && k < K)) store4(o + (int64_t)n * K + k, acc[ki][ni]);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The ring kernels (gemm_tn3_kernel, gemm_tn4_kernel): the same contraction on 192 x 192 tiles with an LDS-DMA ring (no
// register staging, no ds_write).
//
//   block = 512 threads = 8 waves as 4 (n) x 2 (k), wave tile 48 (n) x 96 (k): NI = 3, KI = 6 MFMA tiles, 72 accumulators
//   stage = 64 reduction rows of X[:, k0:k0+192] then of dY[:, n0:n0+192], 384 B per row, 48 KiB; 3 stages, two K-steps of
//           DMA in flight behind the compute (waves 0-3 fetch X, waves 4-7 fetch dY, 6 x 1 KiB DMA pieces each)
//   LDS image: rows are NOT padded (the DMA writes 1 KiB runs); instead the 32-byte granule g of row r sits at
//           g ^ ((r >> 1) & 3).  A 32-lane half of ds_read_b64_tr_b16 takes 8 consecutive rows x 32 B: rows of equal
//           parity differ in (r >> 1) & 3, so they land in 4 different granules of one aligned 128-B group, and odd rows
//           are 32 banks away from even rows (384-B row stride) -> all 64 banks, conflict-free.  The swizzle is applied
//           on the DMA SOURCE address (the LDS destination of a DMA is lane-linear).
//   step:   ONE barrier per step and all eight waves in phase; the fragment reads are software-pipelined ACROSS the barrier:
//               wait DMA(st) | lgkmcnt(0) | barrier | DMA(st+2) -> the stage read during step st-1
//               reads (st, rows 0-31)  interleaved 1:1 with the MFMAs of (st-1, rows 32-63)
//               reads (st, rows 32-63) interleaved 1:1 with the MFMAs of (st,   rows 0-31)
//           Every accumulator sees the same products in the same order in both kernels, so they agree bit for bit.
//   Every Linear of the ViT-S/8 and YAML-decoder shapes has N and K multiples of 192; loads and stores are guarded by column, so
//   other widths that fill their last tile column well enough run here too (ring_shape_ok); the rest use gemm_tn_kernel.
//   Staged bytes per flop are 0.65x those of the 128 x 128 register-staged kernel, and the ds_write_b128 traffic
//   (79 B/clk, the v1 limiter together with the transposed reads) is gone.
// ---------------------------------------------------------------------------------------------------
constexpr int T2 = 192, T2_BR = 64, T2_RS = T2 * 2, T2_HALF = T2_BR * T2_RS, T2_STAGE = 2 * T2_HALF, T2_NSTAGE = 3;
constexpr int T2_GPW = 6, T2_NI = 3, T2_KI = 6, T2_CPR = T2_RS / 16;  // 24 16-byte chunks per row

// One launch can serve TWO weight gradients that share their row count M (the engine pairs fc2 + fc1 and proj + qkv of a
// block): the tiles of both problems form one list, so the M-splits are chosen for the sum.  Alone, the 384 x 384 proj gradient
// needs 64 splits of 18 steps to fill the chip (38 MB of fp32 partials for a 0.6 MB result, 0.47 PF/s); next to qkv it takes
// 16 splits of 70 steps.  `out` / `db` point at the problem's slot inside split 0 of the slab (or at dW / db when there is one
// split); the kernel adds split * split_stride.
struct TnProb {
  const bf16* dY; const bf16* X; float* out; float* db;
  int N, K, tiles_k, tile_begin;
};
struct TnGroup {
  TnProb p[2];
  int nprob, total_tiles;
};

// what one workgroup computes: the 192 x 192 tile at (n0, k0) of its problem over rows [mbeg, mend) = nsteps steps of 64 rows
struct TnTile {
  const bf16* dY; const bf16* X; float* out; float* db;
  int N, K, n0, k0, split, nsteps;
  int64_t mbeg, mend;
};
// XCD-aware order as in gemm_tn_kernel: every tile of one split runs on the same XCD at the same time
__device__ __forceinline__ TnTile tn_tile(const TnGroup& grp, int64_t M, int64_t m_chunk) {
  const int vb = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int gtile = vb % grp.total_tiles;
  const bool second = grp.nprob > 1 && gtile >= grp.p[1].tile_begin;   // workgroup-uniform
  TnTile t;
  t.split = vb / grp.total_tiles;
  t.dY = second ? grp.p[1].dY : grp.p[0].dY;
  t.X = second ? grp.p[1].X : grp.p[0].X;
  t.out = second ? grp.p[1].out : grp.p[0].out;
  t.db = second ? grp.p[1].db : grp.p[0].db;
  t.N = second ? grp.p[1].N : grp.p[0].N;
  t.K = second ? grp.p[1].K : grp.p[0].K;
  const int tiles_k = second ? grp.p[1].tiles_k : grp.p[0].tiles_k;
  const int tile = gtile - (second ? grp.p[1].tile_begin : 0);
  t.n0 = (tile / tiles_k) * T2;
  t.k0 = (tile % tiles_k) * T2;
  t.mbeg = (int64_t)t.split * m_chunk;
  t.mend = t.mbeg + m_chunk < M ? t.mbeg + m_chunk : M;
  t.nsteps = t.mend > t.mbeg ? (int)((t.mend - t.mbeg + T2_BR - 1) / T2_BR) : 0;
  return t;
}

// producer: DMA piece q of this wave covers the lanes' 16-byte chunks c = row * 24 + slot of the operand's 64 x 24 chunks; `sc` is
// the source element offset (inside the tile's row) of the chunk that is stored in `slot`, `width` the columns left in the matrix
struct TnPiece { int row, sc; };
__device__ __forceinline__ TnPiece tn_piece(int wave, int lane, int q, int width) {
  const int c = ((wave & 3) * T2_GPW + q) * 64 + lane;
  const int row = c / T2_CPR, slot = c % T2_CPR;
  int sc = ((((slot >> 1) ^ ((row >> 1) & 3)) << 1) | (slot & 1)) * 8;
  // a last tile column that sticks out of the matrix (widths that are not multiples of 192): its chunks are fetched from the
  // tile's first column instead (valid memory); they only ever reach accumulators whose stores are guarded out in tn_store()
  if (sc >= width) sc = 0;
  return TnPiece{row, sc};
}

template <int N_>
__device__ __forceinline__ void tn_interleave() {   // N_ x (one MFMA, one LDS read)
#if !defined(MAE_DBG_TN3_NOSCHED) && !defined(MAE_DBG_TN_NO_MFMA)   // phase ablation builds (tools/build_dbg_lib.sh tn_no_load tn_no_mfma tn3_nosched): timing probes, wrong values
#pragma unroll
  for (int i = 0; i < N_; ++i) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
  }
#endif
}

// ---- consumer pieces.  A wave holds acc[ki][ni] / accb[ni] and two fragment sets yf[h] / xf[h], one per 32-row half of a step.
// The MFMAs, the bias MFMAs and the declarations they work on are macros (defined here, once) and not functions over array
// references: as functions they changed hipcc's register assignment in the step (tn4: an accumulator that moves to another register
// between the two halves of a step and a hazard s_nop with it; tn3: v_perm re-packing of the fragments in step 0), see
// profiles/r06_wgrad_refactor_isa.txt.  The reads (tn4), the interleave and the epilogue are functions.
// transposed-read offsets inside a stage.  rows 4g + q (+16, +32), 8 bytes at column 4p of a 16-column tile
__device__ __forceinline__ void tn_frag_offsets(int lane, int wn, int wk, int (&yo)[T2_NI], int (&xo)[T2_KI]) {
  const int g = lane >> 4, q4 = (lane & 15) >> 2, p = lane & 3;
  const int sw = ((g & 1) << 1) | (q4 >> 1);  // (row >> 1) & 3 of every row this lane reads
  const int lane_off = (4 * g + q4) * T2_RS + p * 8;
#pragma unroll
  for (int ni = 0; ni < T2_NI; ++ni) yo[ni] = T2_HALF + lane_off + (((wn * T2_NI + ni) ^ sw) * 32);
#pragma unroll
  for (int ki = 0; ki < T2_KI; ++ki) xo[ki] = lane_off + (((wk * T2_KI + ki) ^ sw) * 32);
}
template <int H>
__device__ __forceinline__ bf16x8 tn_frag(const char* p) {
  const bf16x4 lo = lds_read_tr(p + (32 * H) * T2_RS);
  const bf16x4 hi = lds_read_tr(p + (32 * H + 16) * T2_RS);
  return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// fragments [I0, I1) of half H from stage `sb`: 0 .. NI-1 are the dY fragments, NI .. NI+KI-1 the X fragments
template <int H, int I0 = 0, int I1 = T2_NI + T2_KI>
__device__ __forceinline__ void tn_read(const char* sb, const int (&yo)[T2_NI], const int (&xo)[T2_KI], bf16x8 (&yf)[2][T2_NI],
                                        bf16x8 (&xf)[2][T2_KI]) {
#pragma unroll
  for (int i = I0; i < (I1 < T2_NI ? I1 : T2_NI); ++i) yf[H][i] = tn_frag<H>(sb + yo[i]);
#pragma unroll
  for (int i = (I0 > T2_NI ? I0 : T2_NI); i < I1; ++i) xf[H][i - T2_NI] = tn_frag<H>(sb + xo[i - T2_NI]);
}
// accumulators, the bias gradient's set-up, read offsets and fragment sets of a wave: declares acc, accb, do_bias, ones, yo, xo,
// yf, xf from the problem's db pointer and the tile's k0 (and lane, wn, wk of the kernel).
// bias gradient = column sums of dY: one extra MFMA per n-tile against an all-ones operand, done by the waves that own the
// first k tile (do_bias, wave-uniform)
#define TN_WAVE_STATE(db, k0)                                                                               \
  f32x4 acc[T2_KI][T2_NI] = {}, accb[T2_NI] = {};                                                       \
  const bool do_bias = (db) != nullptr && (k0) == 0 && wk == 0;                                         \
  const bf16 one = (bf16)1.0f;                                                                          \
  const bf16x8 ones = bf16x8{one, one, one, one, one, one, one, one};                                   \
  int yo[T2_NI], xo[T2_KI];                                                                             \
  tn_frag_offsets(lane, wn, wk, yo, xo);                                                                \
  bf16x8 yf[2][T2_NI], xf[2][T2_KI];
// the MFMAs of half h for the k tiles [K0, K1)
__device__ __forceinline__ f32x4 tn_mfma1(const bf16x8& x, const bf16x8& y, const f32x4& c) {
#ifdef MAE_DBG_TN_NO_MFMA   // phase ablation build: keep the fragments (and their reads) alive
  asm volatile("" ::"v"(x), "v"(y));
  return c;
#else
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(x, y, c, 0, 0, 0);
#endif
}
#define TN_MFMA(h, K0, K1)                                                                              \
  {                                                                                                     \
    _Pragma("unroll") for (int ki = (K0); ki < (K1); ++ki)                                              \
      _Pragma("unroll") for (int ni = 0; ni < T2_NI; ++ni) acc[ki][ni] = tn_mfma1(xf[h][ki], yf[h][ni], acc[ki][ni]); \
  }
#define TN_BIAS(h)                                                                                      \
  if (do_bias) {                                                                                        \
    _Pragma("unroll") for (int ni = 0; ni < T2_NI; ++ni)                                                \
      accb[ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ones, yf[h][ni], accb[ni], 0, 0, 0);           \
  }
// D[i = k][j = n]: lane holds n = tile col (lane & 15), k = 4 * (lane >> 4) + r -> 16-byte store along k
__device__ __forceinline__ void tn_store(const TnTile& t, int64_t split_stride, int lane, int wn, int wk, bool do_bias,
                                         const f32x4 (&acc)[T2_KI][T2_NI], const f32x4 (&accb)[T2_NI]) {
  float* o = t.out + (int64_t)t.split * split_stride;
  if (do_bias && lane < 16) {  // every row of the ones-product is the same column sum: take row 0
#pragma unroll
    for (int ni = 0; ni < T2_NI; ++ni) {
      const int n = t.n0 + wn * (T2_NI * 16) + ni * 16 + lane;
      if (n < t.N) t.db[(int64_t)t.split * split_stride + n] = accb[ni][0];
    }
  }
#pragma unroll
  for (int ni = 0; ni < T2_NI; ++ni) {
    const int n = t.n0 + wn * (T2_NI * 16) + ni * 16 + (lane & 15);
    float* row = o + (int64_t)n * t.K;
#pragma unroll
    for (int ki = 0; ki < T2_KI; ++ki) {
      const int k = t.k0 + wk * (T2_KI * 16) + ki * 16 + (lane >> 4) * 4;
      if (n < t.N && k < t.K) store4(row + k, acc[ki][ni]);
    }
  }
}
// A 16-byte LDS-DMA from a 64-bit pointer as one opaque instruction pair.  hipcc's waitcnt pass knows that the builtin
// (__builtin_amdgcn_global_load_lds) writes LDS and, because the transposed-read builtin carries no alias information, puts
// `s_waitcnt vmcnt(0)` in front of the first ds_read_b64_tr_b16 after every DMA issue -- which drains the two-steps-ahead ring at
// every step (the DMA phase and the MFMA phase of the wgrad kernel added up for exactly this reason).  Issued from inline asm the
// DMA is invisible to that pass; the counted wait_vm<> + barrier below are what orders it against the reads, checked against the
// all-drained build (MAE_DBG_VMCNT0) like the NT kernel's.  m0 is written behind the compiler's back: nothing else in these
// kernels uses it.
__device__ __forceinline__ void tn_glds16_raw(const bf16* src, char* dst) {
  const uint32_t lds_addr = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)dst);
  // (s_nop 0: an SALU write of m0 needs one wait state before an LDS-DMA reads it; hipcc's hazard recognizer, which inserts
  //  it for the builtin, does not look inside inline asm)
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_addr) : "memory");
}

// ---- tn3: 64-bit-pointer DMA.  Rows past the split's end are clamped to its last row and the dY rows among them zeroed in LDS; the
// production path when a matrix is beyond 32-bit byte offsets (tn4_range_ok), and the reference the tests compare tn4 against
__global__ void __launch_bounds__(512, 2) gemm_tn3_kernel(TnGroup grp, int64_t M, int64_t split_stride, int64_t m_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  // Apart from the producer map, the interleave and the MFMA macros this kernel keeps its own text (tile decode, accumulator and
  // offset set-up, fragment read, step top, epilogue; tn4 uses tn_tile / TN_WAVE_STATE / tn_read / tn_store): each of those, shared,
  // changed instructions of tn3, and with the shared set-up and epilogue it measured 1-1.5 % slower (profiles/r06_wgrad_refactor_*.txt)
  const int vb = (int)xcd_remap(blockIdx.x, gridDim.x);
  const int gtile = vb % grp.total_tiles;
  const int split = vb / grp.total_tiles;
  const bool second = grp.nprob > 1 && gtile >= grp.p[1].tile_begin;   // workgroup-uniform
  const bf16* __restrict__ dY = second ? grp.p[1].dY : grp.p[0].dY;
  const bf16* __restrict__ X = second ? grp.p[1].X : grp.p[0].X;
  float* __restrict__ out = second ? grp.p[1].out : grp.p[0].out;
  float* __restrict__ db = second ? grp.p[1].db : grp.p[0].db;
  const int N = second ? grp.p[1].N : grp.p[0].N, K = second ? grp.p[1].K : grp.p[0].K;
  const int tiles_k = second ? grp.p[1].tiles_k : grp.p[0].tiles_k;
  const int tile = gtile - (second ? grp.p[1].tile_begin : 0);
  const int n0 = (tile / tiles_k) * T2, k0 = (tile % tiles_k) * T2;
  const int64_t mbeg = (int64_t)split * m_chunk;
  const int64_t mend = mbeg + m_chunk < M ? mbeg + m_chunk : M;
  const int nsteps = mend > mbeg ? (int)((mend - mbeg + T2_BR - 1) / T2_BR) : 0;
  const int last_valid = nsteps ? (int)(mend - mbeg - (int64_t)(nsteps - 1) * T2_BR) : 0;  // rows of the last step (1..64)

  const bool isY = wave >= 4;
  const bf16* gbase = isY ? dY + n0 : X + k0;
  const int64_t ld = isY ? N : K;
  int row_[T2_GPW], sc_[T2_GPW];
#pragma unroll
  for (int q = 0; q < T2_GPW; ++q) {
    const TnPiece pc = tn_piece(wave, lane, q, isY ? N - n0 : K - k0);
    row_[q] = pc.row; sc_[q] = pc.sc;
  }
  const bf16 *p0 = gbase + (mbeg + row_[0]) * ld + sc_[0], *p1 = gbase + (mbeg + row_[1]) * ld + sc_[1],
             *p2 = gbase + (mbeg + row_[2]) * ld + sc_[2], *p3 = gbase + (mbeg + row_[3]) * ld + sc_[3],
             *p4 = gbase + (mbeg + row_[4]) * ld + sc_[4], *p5 = gbase + (mbeg + row_[5]) * ld + sc_[5];
  const int64_t inc = (int64_t)T2_BR * ld;
  int is_step = 0, is_stage = 0;
  auto issue = [&]() {
#ifdef MAE_DBG_TN_NO_LOAD
    return;
#endif
    char* dst = smem + is_stage * T2_STAGE + (isY ? T2_HALF : 0) + (wave & 3) * (T2_GPW * 1024);
    if (is_step == nsteps - 1 && last_valid < T2_BR) {
      // ragged last step: rows past the chunk are fetched from its last valid row (finite data, in bounds); the dY rows
      // among them are zeroed in LDS before use, which also removes their X rows from the product
      const int64_t mb = mbeg + (int64_t)is_step * T2_BR;
#pragma unroll
      for (int q = 0; q < T2_GPW; ++q) {
        const int64_t m = mb + (row_[q] < last_valid ? row_[q] : last_valid - 1);
        tn_glds16_raw(gbase + m * ld + sc_[q], dst + q * 1024);
      }
    } else {
      tn_glds16_raw(p0, dst); tn_glds16_raw(p1, dst + 1024); tn_glds16_raw(p2, dst + 2048);
      tn_glds16_raw(p3, dst + 3072); tn_glds16_raw(p4, dst + 4096); tn_glds16_raw(p5, dst + 5120);
      p0 += inc; p1 += inc; p2 += inc; p3 += inc; p4 += inc; p5 += inc;
    }
    is_stage = is_stage == T2_NSTAGE - 1 ? 0 : is_stage + 1;
    ++is_step;
  };

  f32x4 acc[T2_KI][T2_NI], accb[T2_NI];
#pragma unroll
  for (int i = 0; i < T2_KI; ++i)
#pragma unroll
    for (int j = 0; j < T2_NI; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < T2_NI; ++j) accb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool do_bias = db != nullptr && k0 == 0 && wk == 0;
  const bf16 one = (bf16)1.0f;
  const bf16x8 ones = bf16x8{one, one, one, one, one, one, one, one};

  const int g = lane >> 4, q4 = (lane & 15) >> 2, p = lane & 3;
  const int sw = ((g & 1) << 1) | (q4 >> 1);
  const int lane_off = (4 * g + q4) * T2_RS + p * 8;
  int yo[T2_NI], xo[T2_KI];
#pragma unroll
  for (int ni = 0; ni < T2_NI; ++ni) yo[ni] = T2_HALF + lane_off + (((wn * T2_NI + ni) ^ sw) * 32);
#pragma unroll
  for (int ki = 0; ki < T2_KI; ++ki) xo[ki] = lane_off + (((wk * T2_KI + ki) ^ sw) * 32);

  bf16x8 yf[2][T2_NI], xf[2][T2_KI];
#define TN3_READ(sb, h)                                                                                 \
  {                                                                                                     \
    _Pragma("unroll") for (int ni = 0; ni < T2_NI; ++ni) {                                              \
      const bf16x4 lo = lds_read_tr((sb) + yo[ni] + (32 * (h)) * T2_RS);                                \
      const bf16x4 hi = lds_read_tr((sb) + yo[ni] + (32 * (h) + 16) * T2_RS);                           \
      yf[h][ni] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                       \
    }                                                                                                   \
    _Pragma("unroll") for (int ki = 0; ki < T2_KI; ++ki) {                                              \
      const bf16x4 lo = lds_read_tr((sb) + xo[ki] + (32 * (h)) * T2_RS);                                \
      const bf16x4 hi = lds_read_tr((sb) + xo[ki] + (32 * (h) + 16) * T2_RS);                           \
      xf[h][ki] = bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};                       \
    }                                                                                                   \
  }
#define TN3_STEP_TOP(st)                                                                                \
    if ((st) + 1 < nsteps) wait_vm<T2_GPW>(); else wait_vm<0>();                                  \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); /* this wave's reads of the stage refilled below have landed */ \
    __builtin_amdgcn_s_barrier();                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                  \
    asm volatile("" ::: "memory");                                                                      \
    const char* sb = smem + cs * T2_STAGE;                                                              \
    if ((st) == nsteps - 1 && last_valid < T2_BR) {                                                     \
      for (int i = tid; i < (T2_BR - last_valid) * T2_CPR; i += 512)                                    \
        *reinterpret_cast<uint4*>(smem + cs * T2_STAGE + T2_HALF + (last_valid + i / T2_CPR) * T2_RS + (i % T2_CPR) * 16) = uint4{0, 0, 0, 0}; \
      __syncthreads();                                                                                  \
    }                                                                                                   \
    if ((st) + 2 < nsteps) issue();                                                                     \
    __builtin_amdgcn_sched_barrier(0);
  int cs = 0;
  if (nsteps > 0) {
    issue();
    if (nsteps > 1) issue();
    {  // step 0: nothing to multiply yet while the first half is read
      TN3_STEP_TOP(0)
      TN3_READ(sb, 0)
      __builtin_amdgcn_sched_barrier(0);
      TN3_READ(sb, 1)
      TN_MFMA(0, 0, T2_KI)
      tn_interleave<T2_KI * T2_NI>();
      __builtin_amdgcn_sched_barrier(0);
      TN_BIAS(0)
      cs = 1;
    }
    for (int st = 1; st < nsteps; ++st) {
      TN3_STEP_TOP(st)
      TN3_READ(sb, 0)
      TN_MFMA(1, 0, T2_KI)
      tn_interleave<T2_KI * T2_NI>();
      __builtin_amdgcn_sched_barrier(0);
      TN_BIAS(1)
      __builtin_amdgcn_sched_barrier(0);
      TN3_READ(sb, 1)
      TN_MFMA(0, 0, T2_KI)
      tn_interleave<T2_KI * T2_NI>();
      __builtin_amdgcn_sched_barrier(0);
      TN_BIAS(0)
      cs = cs == T2_NSTAGE - 1 ? 0 : cs + 1;
    }
    TN_MFMA(1, 0, T2_KI)
    TN_BIAS(1)
  }
#undef TN3_STEP_TOP
#undef TN3_READ
  float* o = out + (int64_t)split * split_stride;
  if (do_bias && lane < 16) {
#pragma unroll
    for (int ni = 0; ni < T2_NI; ++ni) {
      const int n = n0 + wn * (T2_NI * 16) + ni * 16 + lane;
      if (n < N) db[(int64_t)split * split_stride + n] = accb[ni][0];
    }
  }
#pragma unroll
  for (int ni = 0; ni < T2_NI; ++ni) {
    const int n = n0 + wn * (T2_NI * 16) + ni * 16 + (lane & 15);
#pragma unroll
    for (int ki = 0; ki < T2_KI; ++ki) {
      const int k = k0 + wk * (T2_KI * 16) + ki * 16 + (lane >> 4) * 4;
      if (n < N && k < K) store4(o + (int64_t)n * K + k, acc[ki][ni]);
    }
  }
}
// ---- tn4 (the default): buffer DMA (scalar step offset, range-checked rows), the six pieces of a step issued in pairs between
// thirds of phase A's MFMAs instead of in one burst at the top of the step (BURST: in one burst, for the HBM-bound 192-wide shapes),
// and no special cases in the step
template <bool BURST>
__global__ void __launch_bounds__(512, 2) gemm_tn4_kernel(TnGroup grp, int64_t M, int64_t split_stride, int64_t m_chunk) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wave >> 1, wk = wave & 1;
  const TnTile t = tn_tile(grp, M, m_chunk);
  const int nsteps = t.nsteps;

  // ---- producer side: buffer DMA with one scalar offset per step.  Waves 0-3 fetch X rows, waves 4-7 dY rows; a lane's six
  // (row, chunk) offsets never change; rows past the split's end are out of the descriptor's range and arrive as zeros (no clamp, no
  // zero-fill pass for a ragged last step); the stream is never switched off (phantom pieces past the last step land in a stage
  // nobody reads any more), so every step waits with the same count.
  const bool isY = wave >= 4;
  const uint32_t ldb = (uint32_t)(isY ? t.N : t.K) * 2u;
  const i32x4 rsrc = make_rsrc(isY ? t.dY : t.X, (uint32_t)t.mend * ldb);
  uint32_t vo[T2_GPW];
#pragma unroll
  for (int q = 0; q < T2_GPW; ++q) {
    const TnPiece pc = tn_piece(wave, lane, q, isY ? t.N - t.n0 : t.K - t.k0);
    vo[q] = (uint32_t)pc.row * ldb + (uint32_t)((isY ? t.n0 : t.k0) + pc.sc) * 2u;
  }
  uint32_t soff = (uint32_t)t.mbeg * ldb;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char*)smem) + (uint32_t)((isY ? T2_HALF : 0) + (wave & 3) * (T2_GPW * 1024));
  uint32_t ldst = lds0;
  auto issue_piece = [&](int q) {
#ifndef MAE_DBG_TN_NO_LOAD
    dma16(rsrc, ldst + (uint32_t)(q * 1024), vo[q], soff);
#else
    (void)rsrc; (void)soff; (void)q;
#endif
  };
  auto issue_next = [&]() {
    soff += (uint32_t)T2_BR * ldb;
    ldst = ldst == lds0 + (uint32_t)((T2_NSTAGE - 1) * T2_STAGE) ? lds0 : ldst + (uint32_t)T2_STAGE;
  };

  TN_WAVE_STATE(t.db, t.k0)
  int cs = 0;
  if (nsteps > 0) {
    // two steps of DMA in flight before the first wait
#pragma unroll
    for (int q = 0; q < T2_GPW; ++q) issue_piece(q);
    issue_next();
#pragma unroll
    for (int q = 0; q < T2_GPW; ++q) issue_piece(q);
    issue_next();
    {  // step 0: nothing to multiply yet while the first half is read (the fragments of "the previous half 1" are zeros)
      const bf16 z = (bf16)0.0f;
      const bf16x8 zz = bf16x8{z, z, z, z, z, z, z, z};
#pragma unroll
      for (int ni = 0; ni < T2_NI; ++ni) yf[1][ni] = zz;
#pragma unroll
      for (int ki = 0; ki < T2_KI; ++ki) xf[1][ki] = zz;
    }
    for (int st = 0; st < nsteps; ++st) {
      wait_vm<T2_GPW>();
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this wave's reads of the stage refilled below have landed
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("" ::: "memory");
      const char* sb = smem + cs * T2_STAGE;
      if (BURST) {
#pragma unroll
        for (int q = 0; q < T2_GPW; ++q) issue_piece(q);
        issue_next();
        __builtin_amdgcn_sched_barrier(0);
      }
      // phase A in thirds: three fragments of half 0 are read beside six MFMAs of the previous step's half 1, then two DMA pieces go out
      tn_read<0, 0, T2_NI>(sb, yo, xo, yf, xf); TN_MFMA(1, 0, 2) tn_interleave<6>();
      __builtin_amdgcn_sched_barrier(0);
      if (!BURST) { issue_piece(0); issue_piece(1); }
      __builtin_amdgcn_sched_barrier(0);
      tn_read<0, T2_NI + 0, T2_NI + 3>(sb, yo, xo, yf, xf); TN_MFMA(1, 2, 4) tn_interleave<6>();
      __builtin_amdgcn_sched_barrier(0);
      if (!BURST) { issue_piece(2); issue_piece(3); }
      __builtin_amdgcn_sched_barrier(0);
      tn_read<0, T2_NI + 3, T2_NI + 6>(sb, yo, xo, yf, xf); TN_MFMA(1, 4, 6) tn_interleave<6>();
      __builtin_amdgcn_sched_barrier(0);
      if (!BURST) { issue_piece(4); issue_piece(5); issue_next(); }
      __builtin_amdgcn_sched_barrier(0);
      TN_BIAS(1)
      __builtin_amdgcn_sched_barrier(0);
      // phase B: half 1 is read beside the MFMAs of half 0
      tn_read<1>(sb, yo, xo, yf, xf);
      TN_MFMA(0, 0, T2_KI)
      tn_interleave<T2_KI * T2_NI>();
      __builtin_amdgcn_sched_barrier(0);
      TN_BIAS(0)
      cs = cs == T2_NSTAGE - 1 ? 0 : cs + 1;
    }
    TN_MFMA(1, 0, T2_KI)
    TN_BIAS(1)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the phantom pieces issued past the last step land before the LDS is released
  }
  tn_store(t, split_stride, lane, wn, wk, do_bias, acc, accb);
}
#undef TN_WAVE_STATE
#undef TN_MFMA
#undef TN_BIAS

// ---- host side ------------------------------------------------------------------------------------------------------------

// A/B switches, read per call.  MAE_WGRAD = v1 (register-staged tiles everywhere) | v3r (tn3) | v4 | v4b (tn4 with spread / burst issue)
// for single launches; MAE_WGRAD_PAIR = 0 (two launches) | 3 | 4 | 4b for paired ones.  Anything else selects nothing.
enum class RingSel { Unset, Unknown, Off, Tn3, Tn4, Tn4Burst };
struct RingSelName { const char* text; RingSel sel; };
static const RingSelName kWgradSel[] = {{"v1", RingSel::Off}, {"v3r", RingSel::Tn3}, {"v4", RingSel::Tn4}, {"v4b", RingSel::Tn4Burst}};
static const RingSelName kWgradPairSel[] = {{"0", RingSel::Off}, {"3", RingSel::Tn3}, {"4", RingSel::Tn4}, {"4b", RingSel::Tn4Burst}};
// whole-string match (up to the parent of this file's first commit a prefix was enough: "v1x" pinned v1, "4x" selected tn4)
static RingSel env_sel(const char* var, const RingSelName (&names)[4]) {
  const char* v = getenv(var);
  if (!v || !v[0]) return RingSel::Unset;
  for (const RingSelName& n : names)
    if (!strcmp(v, n.text)) return n.sel;
  return RingSel::Unknown;
}
static RingSel wgrad_sel() { return env_sel("MAE_WGRAD", kWgradSel); }
static RingSel wgrad_pair_sel() { return env_sel("MAE_WGRAD_PAIR", kWgradPairSel); }

// the 192 x 192 ring kernels: every width that is a multiple of 192, and widths that fill their last tile column well enough
// -- 1024 = 5.33 tiles, 512 x 2048 = 3 x 11 tiles at 86 % -- to beat the 128 x 128 register-staged kernel (measured
// 0.55-0.70 PF/s at 1024-wide layers against 0.9 PF/s x fill for this one)
static bool ring_shape_ok(int64_t M, int N, int K) {   // no environment in here: the scratch size depends on it
  if (M < 4096) return false;
  if (N % T2 == 0 && K % T2 == 0) return true;
  if (N % 8 != 0 || K % 8 != 0 || N < T2 || K < T2) return false;
  const int64_t tiles = (int64_t)cdiv(N, T2) * cdiv(K, T2);
  return (int64_t)N * K * 100 >= tiles * T2 * T2 * 75;  // >= 75 % of the tile area is real
}
static int64_t ring_tiles(int N, int K) { return (int64_t)cdiv(N, T2) * cdiv(K, T2); }
// Splits over M for the 192 x 192 ring kernels: one workgroup per CU is resident (144 KiB of LDS), so the launch runs in rounds
// of num_cus() workgroups.  S minimises  rounds(S) x (time of one workgroup at S = 1) / S  +  S x (slab write + read time):
// with few tiles that is the old rule S = CUs / tiles (one full round); with more tiles than half the CUs (1024-wide layers:
// 132 tiles on 256 CUs left 48 % of the chip idle at S = 1) several rounds of shorter workgroups win.
// nk_sum = weight elements of the launch; s_min = 2 for a pair, whose outputs always go through the slab.
static int ring_splits(int64_t M, int64_t tiles, int64_t nk_sum, int s_min) {
  const int64_t cus = num_cus();
  const int64_t smax = std::min<int64_t>(512, std::max<int64_t>(1, M / 256));  // at least 4 reduction steps per block
  const double t1 = (double)M / T2_BR * 1.5;                                    // us: ~1.5 us per 64-row step
  const double slab = (double)nk_sum * 8.0 / 5.0e6;                             // us per split: fp32 partials written once, read once, ~5 TB/s
  int best = s_min;
  double best_cost = 1e30;
  for (int64_t S = s_min; S <= smax; ++S) {
    const double cost = (double)cdiv(tiles * S, cus) * t1 / (double)S + (double)S * slab;
    if (cost < best_cost * 0.999) { best_cost = cost; best = (int)S; }
  }
  return best;
}

// the buffer-DMA kernel addresses a matrix with 32-bit byte offsets (two steps of phantom rows past the end included)
static bool tn4_range_ok(int64_t M, int N, int K) { return (M + 4 * T2_BR) * (int64_t)std::max(N, K) * 2 < ((int64_t)1 << 32); }

// one ring launch over S splits.  Default = tn4 (buffer DMA), burst issue for the 192-wide HBM-bound decoder shapes; tn3 where a
// matrix is beyond 32-bit byte offsets
static int launch_ring(const TnGroup& g, RingSel sel, int64_t M, int S, int64_t stride, int64_t m_chunk, hipStream_t s) {
  bool range_ok = true;
  int wmin = T2 + 1;
  for (int i = 0; i < g.nprob; ++i) {
    range_ok = range_ok && tn4_range_ok(M, g.p[i].N, g.p[i].K);
    wmin = std::min(wmin, std::min(g.p[i].N, g.p[i].K));
  }
  const bool k4 = sel != RingSel::Tn3 && range_ok;
  const bool burst = sel == RingSel::Tn4Burst || (sel != RingSel::Tn4 && wmin <= T2);
  auto kern = k4 ? (burst ? gemm_tn4_kernel<true> : gemm_tn4_kernel<false>) : gemm_tn3_kernel;
  const int lds = T2_NSTAGE * T2_STAGE;
  MAE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)(g.total_tiles * S)), dim3(512), lds, s, g, M, stride, m_chunk);
  MAE_LAUNCH_CHECK();
  return 0;
}

// ordered (deterministic) sum of the per-split slabs: [S][N*K weight partials | N bias partials].
// 256 threads = 32 outputs (float4) x 8 slices of the split index; slice sl adds slabs sl, sl+8, ... and the 8 partial
// sums are combined through LDS in slice order, so the result does not depend on the grid.  (One thread per output
// walking all S slabs serially took 10 us per launch at S = 56 and dominated the small-tile wgrads.)
__global__ void __launch_bounds__(256) slab_reduce_kernel(const float* __restrict__ slabs, int S, int64_t stride4, int64_t nw4,
                                                          int64_t nb4, float* __restrict__ dW, float* __restrict__ db) {
  __shared__ f32x4 red[8][32];
  const int o = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t total = nw4 + nb4;
  for (int64_t base = blockIdx.x * 32ll; base < total; base += (int64_t)gridDim.x * 32) {
    const int64_t i = base + o;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (i < total)
      for (int s = sl; s < S; s += 8) acc += load4(slabs + ((int64_t)s * stride4 + i) * 4);
    red[sl][o] = acc;
    __syncthreads();
    if (sl == 0 && i < total) {
      f32x4 t = red[0][o];
#pragma unroll
      for (int k = 1; k < 8; ++k) t += red[k][o];
      if (i < nw4) store4(dW + i * 4, t); else store4(db + (i - nw4) * 4, t);
    }
    __syncthreads();
  }
}

// the same ordered sum for the slabs of a pair launch: up to four output segments (dW0, db0, dW1, db1) laid out back to back
// inside every split's slab, in float4 units.  (Serving the single launches with this kernel too, as two segments, was tried and
// not shown neutral: on the 3072-wide outputs two of nine rows fell outside the acceptance rule and most medians were 1-3 us higher,
// profiles/r06_wgrad_refactor_ab.txt; so the single launches keep slab_reduce_kernel.)
struct SlabSegs { int64_t end4[4]; float* dst[4]; };
__global__ void __launch_bounds__(256) slab_reduce_group_kernel(const float* __restrict__ slabs, int S, int64_t stride4, SlabSegs sg) {
  __shared__ f32x4 red[8][32];
  const int o = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int64_t total = sg.end4[3];
  for (int64_t base = blockIdx.x * 32ll; base < total; base += (int64_t)gridDim.x * 32) {
    const int64_t i = base + o;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (i < total)
      for (int s = sl; s < S; s += 8) acc += load4(slabs + ((int64_t)s * stride4 + i) * 4);
    red[sl][o] = acc;
    __syncthreads();
    if (sl == 0 && i < total) {
      f32x4 t = red[0][o];
#pragma unroll
      for (int k = 1; k < 8; ++k) t += red[k][o];
      const int seg = i < sg.end4[0] ? 0 : (i < sg.end4[1] ? 1 : (i < sg.end4[2] ? 2 : 3));
      const int64_t b4 = seg == 0 ? 0 : sg.end4[seg - 1];
      store4(sg.dst[seg] + (i - b4) * 4, t);
    }
    __syncthreads();
  }
}

static int wgrad_splits(int64_t M, int N, int K) {
  const int tn = N % 128 == 0 || N % 64 != 0 ? 128 : 64, tk = K % 128 == 0 || K % 64 != 0 ? 128 : 64;  // ragged dims take 128-wide tiles
  const int64_t tiles = (int64_t)cdiv(N, tn) * cdiv(K, tk);
  int64_t S = std::max<int64_t>(1, 512 / tiles);
  S = std::min<int64_t>(S, std::max<int64_t>(1, M / 512));  // at least 8 reduction steps per block
  return (int)std::min<int64_t>(S, 64);
}

int64_t mfma_wgrad_scratch_bytes(int64_t M, int N, int K) {
  if (N % 8 != 0 || K % 8 != 0) return 0;
  int S = wgrad_splits(M, N, K);
  if (ring_shape_ok(M, N, K)) S = std::max(S, ring_splits(M, ring_tiles(N, K), (int64_t)N * K, 1));  // whichever kernel the A/B switch selects at launch time fits
  return S > 1 ? round_up((int64_t)S * ((int64_t)N * K + N) * 4, 256) : 0;
}

template <int NI, int KI, bool RG = false>
static int launch_tn(const bf16* dY, const bf16* X, int64_t M, int N, int K, float* out, float* db, int64_t split_stride, int S,
                     int64_t m_chunk, hipStream_t s) {
  const int tiles_n = (int)cdiv(N, 32 * NI), tiles_k = (int)cdiv(K, 32 * KI);
  const size_t lds = 4 * 64 * TN_RS;
  auto kern = gemm_tn_kernel<NI, KI, RG>;
  MAE_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)(tiles_n * tiles_k * S)), dim3(256), lds, s, dY, X, M, N, K, out, db, split_stride, tiles_n, tiles_k, m_chunk);
  MAE_LAUNCH_CHECK();
  return 0;
}

int mfma_linear_wgrad(const bf16* dY, const bf16* X, int64_t M, int N, int K, float* dW, float* db, void* slab, hipStream_t s) {
  if (N % 8 != 0 || K % 8 != 0 || N < 16 || K < 16 || M < 1) return MFMA_UNSUPPORTED;
  if ((((uintptr_t)dY | (uintptr_t)X | (uintptr_t)dW | (uintptr_t)db | (uintptr_t)slab) & 15) != 0) return MFMA_UNSUPPORTED;
  const RingSel sel = wgrad_sel();
  const bool ring = sel != RingSel::Off && ring_shape_ok(M, N, K);
  const int S = ring ? ring_splits(M, ring_tiles(N, K), (int64_t)N * K, 1) : wgrad_splits(M, N, K);
  if (S > 1 && !slab) return MFMA_UNSUPPORTED;
  const int64_t m_chunk = round_up(cdiv(M, S), 64);
  const int64_t stride = S > 1 ? (int64_t)N * K + N : 0;
  float* out = S > 1 ? reinterpret_cast<float*>(slab) : dW;
  float* dbo = !db ? nullptr : (S > 1 ? out + (int64_t)N * K : db);
  const bool n128 = N % 128 == 0, k128 = K % 128 == 0;
  int r;
  if (ring) {
    TnGroup g{};
    g.p[0] = TnProb{dY, X, out, dbo, N, K, (int)cdiv(K, T2), 0};
    g.nprob = 1; g.total_tiles = (int)ring_tiles(N, K);
    r = launch_ring(g, sel, M, S, stride, m_chunk, s);
  } else if (N % 64 != 0 || K % 64 != 0) {
    r = launch_tn<4, 4, true>(dY, X, M, N, K, out, dbo, stride, S, m_chunk, s);
  } else if (n128 && k128) r = launch_tn<4, 4>(dY, X, M, N, K, out, dbo, stride, S, m_chunk, s);
  else if (n128) r = launch_tn<4, 2>(dY, X, M, N, K, out, dbo, stride, S, m_chunk, s);
  else if (k128) r = launch_tn<2, 4>(dY, X, M, N, K, out, dbo, stride, S, m_chunk, s);
  else r = launch_tn<2, 2>(dY, X, M, N, K, out, dbo, stride, S, m_chunk, s);
  if (r) return r;
  if (S > 1) {
    const int64_t nw4 = (int64_t)N * K / 4, nb4 = db ? N / 4 : 0;
    const int grid = (int)std::min<int64_t>(cdiv(nw4 + nb4, 32), 4096);
    hipLaunchKernelGGL(slab_reduce_kernel, dim3(grid), dim3(256), 0, s, (const float*)slab, S, stride / 4, nw4, nb4, dW, db);
    MAE_LAUNCH_CHECK();
  }
  return 0;
}

// ---- two weight gradients with the same M in one launch (see TnGroup) -------------------------------------------------
static bool wgrad_pair_ok(int64_t M, int N0, int K0, int N1, int K1) {
  // any A/B selection of a single-problem kernel (any non-empty MAE_WGRAD), or MAE_WGRAD_PAIR=0, keeps the launches apart
  if (wgrad_sel() != RingSel::Unset || wgrad_pair_sel() == RingSel::Off) return false;
  return M >= 8192 && ring_shape_ok(M, N0, K0) && ring_shape_ok(M, N1, K1) && N0 % 4 == 0 && N1 % 4 == 0;
}
int64_t mfma_wgrad_pair_scratch_bytes(int64_t M, int N0, int K0, int N1, int K1) {
  if (M < 8192 || !ring_shape_ok(M, N0, K0) || !ring_shape_ok(M, N1, K1)) return 0;
  const int64_t per = (int64_t)N0 * K0 + N0 + (int64_t)N1 * K1 + N1;
  return round_up((int64_t)ring_splits(M, ring_tiles(N0, K0) + ring_tiles(N1, K1), (int64_t)N0 * K0 + (int64_t)N1 * K1, 2) * per * 4, 256);
}
int mfma_linear_wgrad_pair(const bf16* dY0, const bf16* X0, int N0, int K0, float* dW0, float* db0, const bf16* dY1, const bf16* X1,
                           int N1, int K1, float* dW1, float* db1, int64_t M, void* slab, hipStream_t s) {
  if (!wgrad_pair_ok(M, N0, K0, N1, K1) || !slab || !db0 || !db1) return MFMA_UNSUPPORTED;
  if ((((uintptr_t)dY0 | (uintptr_t)X0 | (uintptr_t)dW0 | (uintptr_t)db0 | (uintptr_t)dY1 | (uintptr_t)X1 | (uintptr_t)dW1 | (uintptr_t)db1 |
        (uintptr_t)slab) & 15) != 0)
    return MFMA_UNSUPPORTED;
  const int t0 = (int)ring_tiles(N0, K0), t1 = (int)ring_tiles(N1, K1);
  const int64_t nk0 = (int64_t)N0 * K0, nk1 = (int64_t)N1 * K1;
  const int S = ring_splits(M, (int64_t)t0 + t1, nk0 + nk1, 2);
  const int64_t m_chunk = round_up(cdiv(M, S), 64);
  const int64_t stride = nk0 + N0 + nk1 + N1;   // floats per split: [dW0 | db0 | dW1 | db1]
  float* base = reinterpret_cast<float*>(slab);
  TnGroup g{};
  g.p[0] = TnProb{dY0, X0, base, base + nk0, N0, K0, (int)cdiv(K0, T2), 0};
  g.p[1] = TnProb{dY1, X1, base + nk0 + N0, base + nk0 + N0 + nk1, N1, K1, (int)cdiv(K1, T2), t0};
  g.nprob = 2; g.total_tiles = t0 + t1;
  MAE_TRY(launch_ring(g, wgrad_pair_sel(), M, S, stride, m_chunk, s));
  SlabSegs sg;
  sg.end4[0] = nk0 / 4; sg.end4[1] = sg.end4[0] + N0 / 4; sg.end4[2] = sg.end4[1] + nk1 / 4; sg.end4[3] = sg.end4[2] + N1 / 4;
  sg.dst[0] = dW0; sg.dst[1] = db0; sg.dst[2] = dW1; sg.dst[3] = db1;
  const int grid = (int)std::min<int64_t>(cdiv(sg.end4[3], 32), 4096);
  hipLaunchKernelGGL(slab_reduce_group_kernel, dim3(grid), dim3(256), 0, s, (const float*)slab, S, stride / 4, sg);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae
