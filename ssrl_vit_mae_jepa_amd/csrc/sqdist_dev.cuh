// The difference-form pairwise squared distances shared by k_tsne.hip and k_umap.hip.  Both objects are built
// with -ffp-contract=off; the one fused multiply-add per term is written as fmaf.  The kernel has internal linkage: each object
// carries its own copy of the same code.
#pragma once
#include "kernels.h"

namespace mae {

constexpr int TS_THREADS = 256;
constexpr int TS_TILE = 64, TS_KC = 16, TS_KS = TS_TILE + 4;   // sqdist: tile edge, staged columns, k-major row stride

// d_ij = sum_k (x_ik - x_jk)^2 in the order of k into P (n, pitch) and, if given, sqdist (n, n).  Grid (ceil(n / 64), ceil(n / 64)).
static __global__ void __launch_bounds__(TS_THREADS) tsne_sqdist_kernel(const float* __restrict__ x, int n, int dim, float* __restrict__ P, int pitch,
                                                                        float* __restrict__ sqdist) {
  __shared__ __attribute__((aligned(16))) float As[TS_KC * TS_KS], Bs[TS_KC * TS_KS];
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int i0 = blockIdx.y * TS_TILE, j0 = blockIdx.x * TS_TILE;
  float acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.f;
  const int kk = t & 15, r0 = t >> 4;   // staging: 16 consecutive columns of one row per 16 lanes
  for (int k0 = 0; k0 < dim; k0 += TS_KC) {
    __syncthreads();   // the previous chunk has been read
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int r = r0 + 16 * p, k = k0 + kk;
      const int ri = i0 + r, rj = j0 + r;
      As[kk * TS_KS + r] = (ri < n && k < dim) ? x[(int64_t)ri * dim + k] : 0.f;   // zeros past n and past dim: a difference of 0
      Bs[kk * TS_KS + r] = (rj < n && k < dim) ? x[(int64_t)rj * dim + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TS_KC; ++k) {
      const f32x4 a = load4(As + k * TS_KS + 4 * ty), b = load4(Bs + k * TS_KS + 4 * tx);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float df = a[u] - b[v];
          acc[u][v] = fmaf(df, df, acc[u][v]);
        }
    }
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = i0 + 4 * ty + u;
    if (i >= n) continue;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int j = j0 + 4 * tx + v;
      if (j >= n) continue;
      P[(int64_t)i * pitch + j] = acc[u][v];
      if (sqdist) sqdist[(int64_t)i * n + j] = acc[u][v];
    }
  }
}

}  // namespace mae
