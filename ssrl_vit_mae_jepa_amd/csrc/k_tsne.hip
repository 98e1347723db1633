// Exact t-SNE of n <= 16384 feature rows in the plane: affinities, gradient and the descent step.  Everything is
// fp32, every sum has an order fixed by (n, dim) alone, there are no atomics, nothing synchronises with the host, and every buffer is
// the caller's.  This object is compiled with -ffp-contract=off (Makefile): a product followed by a sum is two roundings unless it is
// written as fmaf, so the descent step can be restated in numpy fp32 bit for bit and every fused multiply-add below is one on purpose.
//
// P lives in an (n, pitch) buffer, pitch = round_up(n, 4) (mae_tsne_pitch), so that every row starts 16-byte aligned; the columns
// [n, pitch) hold zeros.
//
// Affinities, three launches, the P buffer itself being the only working space:
//   tsne_sqdist_kernel   d_ij = sum_k (x_ik - x_jk)^2 in the order of k, one fmaf per term: a 64 x 64 tile of pairs per workgroup, 4 x 4
//                        per thread, x staged through LDS 16 columns at a time, k-major ([16][68]: the float4 reads of a thread's four
//                        rows are aligned, the 16 lanes that share them broadcast; the staging ds_write_b32 is 2-way conflicted, which
//                        costs nothing).  (a - b)^2 = (b - a)^2 exactly, so d is symmetric bit for bit.  Written into the P buffer.
//   tsne_search_kernel   one workgroup per row.  The row of distances, less its minimum over j != i, stays in LDS (n floats <= 64 KiB)
//                        for sklearn's _binary_search_perplexity: beta from 1, doubled or halved until bracketed, then bisected, at most
//                        100 steps, until |H - log(perplexity)| <= 1e-5 with H = log S + beta T / S, S = sum_{j != i} e^(-beta d'_j),
//                        T = sum d'_j e^(-beta d'_j).  The minimum's own term is e^0 = 1, so S >= 1 and no row underflows.  Thread t sums
//                        j = t, t + 256, ... in order, then the xor butterfly, then the four waves in order: every thread holds the
//                        same S and T and takes the same branch.  One code path for every n.  The row of p_j|i = e_j / S replaces the
//                        distances in place.
//   tsne_symmetrise_kernel  P_ij = (p_j|i + p_i|j) / (2 n) in place: a workgroup loads the 64 x 64 tiles (I, J) and (J, I), I <= J,
//                        into LDS and writes both back.  The sum commutes, so P is symmetric bit for bit; the diagonal is 0 + 0.
//
// Gradient: tsne_gradient_kernel streams P once.  A wave owns four consecutive rows over the whole column range (no column slices: at
// n = 2000 that is 125 workgroups and the call is launch-bound anyway, at 16384 it is 1024); lane l takes the columns 4 l + 256 k + e,
// e = 0..3, as one 16-byte load per row (inside the pitch: the padding columns are read, not used; the next trip's
// loads are issued before this trip's arithmetic), and the four rows share the lane's two 16-byte loads of y (8 n bytes of y from L2 per wave
// against 16 n of P).  Per pair: w = v_rcp(1 + |y_i - y_j|^2), a += (p w) dy, r += w^2 dy, z += w (j != i), each lane in the order of
// its columns, then the xor butterfly.  tsne_finalize_kernel adds the n row sums z_i in a fixed order (thread t: t, t + 256, ...;
// butterfly; waves in order -- every workgroup does the same sum and gets the same Z), forms grad = 4 (alpha a - r / Z) and, in
// mae_tsne_step, applies the descent step in the same launch: two launches per iteration.
#include "sqdist_dev.cuh"

namespace mae {

constexpr int TS_MIN_N = 8, TS_MAX_N = 16384, TS_MAX_DIM = 8192;
constexpr int TS_ROWS = 4;                                     // gradient: rows of a wave
constexpr int TS_MAX_STEPS = 100;
constexpr float TS_TOL = 1e-5f;

static bool tsne_n_ok(int n) { return n >= TS_MIN_N && n <= TS_MAX_N; }
int tsne_pitch(int n) { return tsne_n_ok(n) ? (int)round_up(n, 4) : -1; }
// gradient scratch: a (n, 2), r (n, 2), z (n), kl rows (n), each padded to a multiple of 4 floats
int64_t tsne_scratch_bytes(int n, int dim) {
  if (!tsne_n_ok(n) || dim < 1 || dim > TS_MAX_DIM) return -1;
  return 6 * round_up(n, 4) * (int64_t)sizeof(float);
}

// ---- affinities ----------------------------------------------------------------------------------------------------------
// tsne_sqdist_kernel: sqdist_dev.cuh (shared with k_umap.hip)

// (a, b) summed over the 256 threads; red = 8 floats of LDS; the same bits in every thread
__device__ __forceinline__ void block_sum2_256(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[w] = a;
    red[4 + w] = b;
  }
  __syncthreads();
  a = ((red[0] + red[1]) + red[2]) + red[3];
  b = ((red[4] + red[5]) + red[6]) + red[7];
}

// LDS: d[round_up(n, 4)], then red[8]
__global__ void __launch_bounds__(TS_THREADS) tsne_search_kernel(float* __restrict__ P, int pitch, int n, float desired, float* __restrict__ beta_out,
                                                                 float* __restrict__ p_cond) {
  extern __shared__ __attribute__((aligned(16))) float ts_lds[];
  float* d = ts_lds;
  float* red = ts_lds + pitch;
  const int t = threadIdx.x, i = blockIdx.x;
  float* row = P + (int64_t)i * pitch;
  float m = INFINITY;
  for (int j = t; j < n; j += TS_THREADS) {
    const float v = row[j];
    d[j] = v;
    if (j != i) m = fminf(m, v);
  }
  m = wave_max(-m);
  if ((t & 63) == 0) red[t >> 6] = m;
  __syncthreads();
  m = -fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));   // the row minimum over j != i; the next write of red follows a barrier
  for (int j = t; j < n; j += TS_THREADS) d[j] -= m;           // a thread reads back only what it wrote
  float beta = 1.f, lo = -INFINITY, hi = INFINITY, S = 1.f;
  for (int step = 0; step < TS_MAX_STEPS; ++step) {
    float s = 0.f, td = 0.f;
    for (int j = t; j < n; j += TS_THREADS) {
      if (j == i) continue;
      const float e = __expf(-beta * d[j]);
      s += e;
      td = fmaf(d[j], e, td);
    }
    block_sum2_256(s, td, red);
    S = s;
    const float diff = (logf(s) + beta * (td / s)) - desired;
    if (fabsf(diff) <= TS_TOL || step == TS_MAX_STEPS - 1) break;   // uniform: every thread holds the same sums
    if (diff > 0.f) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
    }
  }
  for (int j = t; j < pitch; j += TS_THREADS) {
    const float p = (j == i || j >= n) ? 0.f : __expf(-beta * d[j]) / S;
    row[j] = p;
    if (p_cond && j < n) p_cond[(int64_t)i * n + j] = p;
  }
  if (beta_out && t == 0) beta_out[i] = beta;
}

__global__ void __launch_bounds__(TS_THREADS) tsne_symmetrise_kernel(float* __restrict__ P, int pitch, int n, float two_n) {
  if (blockIdx.x < blockIdx.y) return;   // the pair (I, J), I <= J, is one workgroup's
  __shared__ float A[TS_TILE * (TS_TILE + 1)], B[TS_TILE * (TS_TILE + 1)];
  const int i0 = blockIdx.y * TS_TILE, j0 = blockIdx.x * TS_TILE;
  const int c = threadIdx.x & 63, r0 = threadIdx.x >> 6;
  for (int r = r0; r < TS_TILE; r += 4) {
    A[r * (TS_TILE + 1) + c] = (i0 + r < n && j0 + c < n) ? P[(int64_t)(i0 + r) * pitch + j0 + c] : 0.f;
    B[r * (TS_TILE + 1) + c] = (j0 + r < n && i0 + c < n) ? P[(int64_t)(j0 + r) * pitch + i0 + c] : 0.f;
  }
  __syncthreads();
  for (int r = r0; r < TS_TILE; r += 4) {
    if (i0 + r < n && j0 + c < n) P[(int64_t)(i0 + r) * pitch + j0 + c] = (A[r * (TS_TILE + 1) + c] + B[c * (TS_TILE + 1) + r]) / two_n;
    if (i0 != j0 && j0 + r < n && i0 + c < n) P[(int64_t)(j0 + r) * pitch + i0 + c] = (A[c * (TS_TILE + 1) + r] + B[r * (TS_TILE + 1) + c]) / two_n;
  }
}

static int check_tsne_n(int n, const char* who) {
  MAE_REQUIRE(tsne_n_ok(n), "%s: n = %d outside [%d, %d]", who, n, TS_MIN_N, TS_MAX_N);
  return 0;
}

int launch_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* sqdist, float* beta, float* p_cond, hipStream_t s) {
  const char* who = "tsne_affinities";
  MAE_TRY(check_tsne_n(n, who));
  MAE_REQUIRE(dim >= 1 && dim <= TS_MAX_DIM, "%s: dim = %d outside [1, %d]", who, dim, TS_MAX_DIM);
  MAE_REQUIRE(perplexity >= 1.f && perplexity < (float)(n - 1), "%s: perplexity = %g outside [1, n - 1 = %d)", who, (double)perplexity, n - 1);
  MAE_REQUIRE(x && P, "%s: null x / P", who);
  MAE_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)P & 15) == 0 && ((uintptr_t)sqdist & 3) == 0 && ((uintptr_t)beta & 3) == 0 && ((uintptr_t)p_cond & 3) == 0,
              "%s: P must be 16-byte aligned, every other buffer 4-byte", who);
  const int pitch = tsne_pitch(n), nb = (int)cdiv(n, TS_TILE);
  hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(nb, nb), dim3(TS_THREADS), 0, s, x, n, dim, P, pitch, sqdist);
  MAE_LAUNCH_CHECK();
  const size_t lds = (size_t)(pitch + 8) * sizeof(float);
  MAE_TRY(allow_lds(tsne_search_kernel, lds));
  hipLaunchKernelGGL(tsne_search_kernel, dim3(n), dim3(TS_THREADS), lds, s, P, pitch, n, (float)log((double)perplexity), beta, p_cond);
  MAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(tsne_symmetrise_kernel, dim3(nb, nb), dim3(TS_THREADS), 0, s, P, pitch, n, 2.f * (float)n);
  MAE_LAUNCH_CHECK();
  return 0;
}

// ---- gradient --------------------------------------------------------------------------------------------------------------
template <bool KL>
__global__ void __launch_bounds__(TS_THREADS) tsne_gradient_kernel(const float* __restrict__ P, int pitch, const float* __restrict__ y, int n,
                                                                   float* __restrict__ a_out, float* __restrict__ r_out, float* __restrict__ z_out,
                                                                   float* __restrict__ kl_out) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row0 = (blockIdx.x * (TS_THREADS / 64) + wv) * TS_ROWS;
  if (row0 >= n) return;   // the wave's own rows: no barrier follows
  int ri[TS_ROWS];
  float yix[TS_ROWS], yiy[TS_ROWS], ax[TS_ROWS], ay[TS_ROWS], rx[TS_ROWS], ry[TS_ROWS], z[TS_ROWS], kl[TS_ROWS];
  const float* prow[TS_ROWS];
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) {
    ri[r] = min(row0 + r, n - 1);   // a row past n repeats the last one and is not stored
    yix[r] = y[2 * ri[r]];
    yiy[r] = y[2 * ri[r] + 1];
    prow[r] = P + (int64_t)ri[r] * pitch;
    ax[r] = ay[r] = rx[r] = ry[r] = z[r] = kl[r] = 0.f;
  }
  f32x4 p[TS_ROWS], pn[TS_ROWS];
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) p[r] = 4 * lane < pitch ? load4(prow[r] + 4 * lane) : f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j0 = 4 * lane; j0 < pitch; j0 += 4 * 64) {
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r)   // the next trip's 16 bytes of every row are in flight while this trip computes
      pn[r] = j0 + 4 * 64 < pitch ? load4(prow[r] + j0 + 4 * 64) : f32x4{0.f, 0.f, 0.f, 0.f};
    float yjx[4], yjy[4];
    bool valid[4];
    if (j0 + 4 <= n) {
      const f32x4 u = load4(y + 2 * j0), v = load4(y + 2 * j0 + 4);
      yjx[0] = u[0], yjy[0] = u[1], yjx[1] = u[2], yjy[1] = u[3], yjx[2] = v[0], yjy[2] = v[1], yjx[3] = v[2], yjy[3] = v[3];
      valid[0] = valid[1] = valid[2] = valid[3] = true;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        valid[e] = j0 + e < n;
        yjx[e] = valid[e] ? y[2 * (j0 + e)] : 0.f;
        yjy[e] = valid[e] ? y[2 * (j0 + e) + 1] : 0.f;
      }
    }
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool on = valid[e] && j0 + e != ri[r];
        const float dx = valid[e] ? yix[r] - yjx[e] : 0.f, dy = valid[e] ? yiy[r] - yjy[e] : 0.f;
        const float q = fmaf(dx, dx, fmaf(dy, dy, 1.f));
        const float w = v_rcp(q);
        const float pe = valid[e] ? p[r][e] : 0.f;
        const float pw = pe * w, w2 = w * w;
        ax[r] = fmaf(pw, dx, ax[r]);
        ay[r] = fmaf(pw, dy, ay[r]);
        rx[r] = fmaf(w2, dx, rx[r]);
        ry[r] = fmaf(w2, dy, ry[r]);
        z[r] += on ? w : 0.f;
        if (KL) {
          if (on && pe > 0.f) kl[r] = fmaf(pe, logf(pe) + logf(q), kl[r]);   // -log w = log q; 0 log 0 = 0
        }
      }
#pragma unroll
    for (int r = 0; r < TS_ROWS; ++r) p[r] = pn[r];
  }
#pragma unroll
  for (int r = 0; r < TS_ROWS; ++r) {
    const float sax = wave_sum(ax[r]), say = wave_sum(ay[r]), srx = wave_sum(rx[r]), sry = wave_sum(ry[r]), sz = wave_sum(z[r]);
    const float skl = KL ? wave_sum(kl[r]) : 0.f;
    if (lane == 0 && row0 + r < n) {
      const int i = row0 + r;
      a_out[2 * i] = sax, a_out[2 * i + 1] = say, r_out[2 * i] = srx, r_out[2 * i + 1] = sry, z_out[i] = sz;
      if (KL) kl_out[i] = skl;
    }
  }
}

// sklearn's _gradient_descent step on one coordinate: every operation rounds once (this object is built with -ffp-contract=off)
__device__ __forceinline__ void tsne_descend(float g, float& y, float& u, float& gain, float momentum, float lr, float min_gain) {
  gain = u * g < 0.f ? gain + 0.2f : gain * 0.8f;
  gain = fmaxf(gain, min_gain);
  const float gg = g * gain;
  u = momentum * u - lr * gg;
  y = y + u;
}

// the sum of v[0 .. n) in the order every workgroup shares: thread t adds t, t + 256, ...; butterfly; waves in order
__device__ __forceinline__ float tsne_ordered_sum(const float* __restrict__ v, int n, float* red) {
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += TS_THREADS) s += v[i];
  return block_sum_256(s, red);
}

template <bool UPDATE>
__global__ void __launch_bounds__(TS_THREADS) tsne_finalize_kernel(const float* __restrict__ a, const float* __restrict__ r, const float* __restrict__ z,
                                                                   const float* __restrict__ klrow, int n, float alpha, float* __restrict__ grad,
                                                                   float* __restrict__ kl, float* __restrict__ y, float* __restrict__ upd,
                                                                   float* __restrict__ gains, float momentum, float lr, float min_gain) {
  __shared__ float red[4];
  const float Z = tsne_ordered_sum(z, n, red);
  if (kl && blockIdx.x == 0) {   // uniform over the workgroup
    const float k = tsne_ordered_sum(klrow, n, red);
    if (threadIdx.x == 0) kl[0] = k + logf(Z);
  }
  const int e = blockIdx.x * TS_THREADS + threadIdx.x;   // one coordinate of one point
  if (e >= 2 * n) return;
  const float g = 4.f * fmaf(alpha, a[e], -(r[e] / Z));
  grad[e] = g;
  if (UPDATE) {
    float yv = y[e], uv = upd[e], gv = gains[e];
    tsne_descend(g, yv, uv, gv, momentum, lr, min_gain);
    y[e] = yv, upd[e] = uv, gains[e] = gv;
  }
}

__global__ void __launch_bounds__(TS_THREADS) tsne_update_kernel(float* __restrict__ y, float* __restrict__ upd, float* __restrict__ gains,
                                                                 const float* __restrict__ grad, int n2, float momentum, float lr, float min_gain) {
  const int e = blockIdx.x * TS_THREADS + threadIdx.x;
  if (e >= n2) return;
  float yv = y[e], uv = upd[e], gv = gains[e];
  tsne_descend(grad[e], yv, uv, gv, momentum, lr, min_gain);
  y[e] = yv, upd[e] = uv, gains[e] = gv;
}

static int check_descent(const char* who, const float* y, const float* upd, const float* gains, const float* grad) {
  MAE_REQUIRE(y && upd && gains && grad, "%s: null y / update / gains / grad", who);
  MAE_REQUIRE((((uintptr_t)y | (uintptr_t)upd | (uintptr_t)gains | (uintptr_t)grad) & 15) == 0, "%s: every buffer must be 16-byte aligned", who);
  return 0;
}

// the gradient pass and its finalising launch; y_io != null: the descent step in the finalising launch
static int run_gradient(const char* who, const float* P, const float* y, int n, float alpha, float* grad, float* kl, void* scratch, int64_t scratch_bytes,
                        float* y_io, float* upd, float* gains, float momentum, float lr, float min_gain, hipStream_t s) {
  MAE_TRY(check_tsne_n(n, who));
  MAE_REQUIRE(P && y && grad && scratch, "%s: null P / y / grad / scratch", who);
  MAE_REQUIRE((((uintptr_t)P | (uintptr_t)y | (uintptr_t)grad | (uintptr_t)scratch) & 15) == 0 && ((uintptr_t)kl & 3) == 0,
              "%s: P, y, grad and scratch must be 16-byte aligned", who);
  const int64_t need = tsne_scratch_bytes(n, 1);
  MAE_REQUIRE(scratch_bytes >= need, "%s: scratch_bytes = %lld below mae_tsne_scratch_bytes = %lld", who, (long long)scratch_bytes, (long long)need);
  const int np = (int)round_up(n, 4), pitch = tsne_pitch(n);
  float* a = (float*)scratch;
  float *r = a + 2 * np, *z = r + 2 * np, *klrow = z + np;
  const dim3 grid((unsigned)cdiv(n, TS_ROWS * (TS_THREADS / 64)));
  with_bool(kl != nullptr, [&](auto b) {
    hipLaunchKernelGGL(tsne_gradient_kernel<decltype(b)::value>, grid, dim3(TS_THREADS), 0, s, P, pitch, y, n, a, r, z, klrow);
  });
  MAE_LAUNCH_CHECK();
  const dim3 fgrid((unsigned)cdiv(2 * n, TS_THREADS));
  with_bool(y_io != nullptr, [&](auto b) {
    hipLaunchKernelGGL(tsne_finalize_kernel<decltype(b)::value>, fgrid, dim3(TS_THREADS), 0, s, (const float*)a, (const float*)r, (const float*)z,
                       (const float*)klrow, n, alpha, grad, kl, y_io, upd, gains, momentum, lr, min_gain);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_tsne_gradient(const float* P, const float* y, int n, float alpha, float* grad, float* kl, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  return run_gradient("tsne_gradient", P, y, n, alpha, grad, kl, scratch, scratch_bytes, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, s);
}

int launch_tsne_update(float* y, float* upd, float* gains, const float* grad, int n, float momentum, float lr, float min_gain, hipStream_t s) {
  const char* who = "tsne_update";
  MAE_TRY(check_tsne_n(n, who));
  MAE_TRY(check_descent(who, y, upd, gains, grad));
  hipLaunchKernelGGL(tsne_update_kernel, dim3((unsigned)cdiv(2 * n, TS_THREADS)), dim3(TS_THREADS), 0, s, y, upd, gains, grad, 2 * n, momentum, lr, min_gain);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_tsne_step(const float* P, float* y, float* upd, float* gains, int n, float alpha, float momentum, float lr, float min_gain, float* grad,
                     float* kl, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  const char* who = "tsne_step";
  MAE_TRY(check_tsne_n(n, who));
  MAE_TRY(check_descent(who, y, upd, gains, grad));
  return run_gradient(who, P, y, n, alpha, grad, kl, scratch, scratch_bytes, y, upd, gains, momentum, lr, min_gain, s);
}

}  // namespace mae

extern "C" int32_t mae_tsne_pitch(int32_t n) { return mae::tsne_pitch(n); }
extern "C" int64_t mae_tsne_scratch_bytes(int32_t n, int32_t dim) { return mae::tsne_scratch_bytes(n, dim); }
extern "C" int mae_tsne_affinities(const float* x, int32_t n, int32_t dim, float perplexity, float* P, float* sqdist, float* beta, float* p_cond,
                                   void* stream) {
  return mae::launch_tsne_affinities(x, n, dim, perplexity, P, sqdist, beta, p_cond, (hipStream_t)stream);
}
extern "C" int mae_tsne_gradient(const float* P, const float* y, int32_t n, float alpha, float* grad, float* kl, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  return mae::launch_tsne_gradient(P, y, n, alpha, grad, kl, scratch, scratch_bytes, (hipStream_t)stream);
}
extern "C" int mae_tsne_update(float* y, float* update, float* gains, const float* grad, int32_t n, float momentum, float learning_rate, float min_gain,
                               void* stream) {
  return mae::launch_tsne_update(y, update, gains, grad, n, momentum, learning_rate, min_gain, (hipStream_t)stream);
}
extern "C" int mae_tsne_step(const float* P, float* y, float* update, float* gains, int32_t n, float alpha, float momentum, float learning_rate,
                             float min_gain, float* grad, float* kl, void* scratch, int64_t scratch_bytes, void* stream) {
  return mae::launch_tsne_step(P, y, update, gains, n, alpha, momentum, learning_rate, min_gain, grad, kl, scratch, scratch_bytes, (hipStream_t)stream);
}
