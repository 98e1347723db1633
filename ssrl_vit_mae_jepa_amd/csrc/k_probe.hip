// The linear probe's two kernels (MAE paper A.1, Table 10; I-JEPA's probe): BatchNorm1d(affine=False) over cached feature rows and the
// LARS step of the head.  The step's logits, loss, dW and db are mae_classifier_head on the normalised rows (k_classifier.hip).
// Reference behaviour:
//   batchnorm == torch.nn.BatchNorm1d(dim, affine=False, eps) in train / eval mode (biased variance in y, unbiased in running_var)
//   lars      == the LARS of the MAE code base (util/lars.py): dp = g + wd p; q = tc |p| / |dp| where both norms are positive, else 1;
//                mu = momentum mu + dp q; p -= lr mu.  1-D tensors (adapt = 0) take neither weight decay nor the trust ratio.
// Both are bandwidth-bound streams of float4.  Every sum has a fixed order that depends on the shape alone; there are no atomics.
//
// BatchNorm geometry.  d4 = dim / 4 float4 columns; a block of 256 threads covers RP = 256 / d4 whole rows per trip (thread t < RP d4
// holds float4 column t % d4 of row slot t / d4, so consecutive threads read consecutive float4, across row ends too).  Block b owns
// the contiguous rows [b S, (b + 1) S), S a multiple of RP, and walks them S / RP trips; the RP row slots are added in order through
// LDS into partial[b][dim]; launch_sum_partials adds the blocks.  Two such column reductions run, both centred:
//   pass 0   S0[c] = sum_r (x[r][c] - x[0][c])                    mean[c] = x[0][c] + S0[c] / rows
//   pass 1   M2[c] = sum_r (x[r][c] - mean[c])^2                  var[c]  = M2[c] / rows
// then one sweep writes y = (x - mean) rsqrt(var + eps).  x is read three times and y written once.  The pivot row makes a constant
// column exact (every difference is 0, so mean = x[0][c], M2 = 0 and y = 0 bit for bit) and keeps the first sum's terms the size of the
// spread, not of the mean.  The normalising sweep takes mean from the scratch, never from x, so y may be x itself.
#include "kernels.h"
#include "lars_dev.cuh"

namespace mae {

constexpr int BN_MAX_BLOCKS = 1024;  // row slices of the column reductions
constexpr int BN_MIN_TRIPS = 4;      // trips a block makes at least before another block is opened
constexpr int BN_NORM_BLOCKS = 256 * 16;

struct BnGeo {
  int d4, rp, grid;
  int64_t slice;  // rows per block, a multiple of rp
};
static BnGeo bn_geometry(int64_t rows, int dim) {
  BnGeo g;
  g.d4 = dim / 4;
  g.rp = 256 / g.d4;
  const int64_t want = std::min<int64_t>(cdiv(rows, (int64_t)g.rp * BN_MIN_TRIPS), BN_MAX_BLOCKS);
  g.slice = round_up(cdiv(rows, want), g.rp);
  g.grid = (int)cdiv(rows, g.slice);
  return g;
}

// PASS 0: partial[b][c] = sum over the block's rows of x - x[0]; PASS 1: of (x - mean)^2, mean = x[0] + s0 / rows (block 0 stores it)
template <int PASS>
__global__ void __launch_bounds__(256) bn_colsum_kernel(const float* __restrict__ x, const float* __restrict__ s0, int64_t rows, int dim,
                                                        int rp, int64_t slice, float* __restrict__ mean_out, float* __restrict__ partial) {
  __shared__ __attribute__((aligned(16))) f32x4 red[256];
  const int d4 = dim >> 2, t = threadIdx.x;
  const bool active = t < rp * d4;
  const int c = t % d4, rs = t / d4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (active) {
    f32x4 ref = load4(x + c * 4);
    if (PASS == 1) {
      ref += load4(s0 + c * 4) / (float)rows;
      if (blockIdx.x == 0 && rs == 0) store4(mean_out + c * 4, ref);
    }
    const int64_t lo = blockIdx.x * slice, hi = lo + slice < rows ? lo + slice : rows;
#pragma unroll 4
    for (int64_t r = lo + rs; r < hi; r += rp) {
      const f32x4 d = load4(x + r * dim + c * 4) - ref;
      if (PASS == 0) acc += d; else acc += d * d;
    }
    red[t] = acc;
  }
  __syncthreads();
  if (t < d4) {
    f32x4 v = red[t];
    for (int j = 1; j < rp; ++j) v += red[j * d4 + t];
    store4(partial + (int64_t)blockIdx.x * dim + t * 4, v);
  }
}

// TRAIN: mean / m2 are the scratch's statistics; else the running buffers.  Block 0 writes the statistics out and, when tracked, the
// running buffers: rm' = (1 - mom) rm + mom mean, rv' = (1 - mom) rv + mom m2 / (rows - 1).  x and y may be the same buffer.
// SWEEP = false (mae_batchnorm_stats) is the same statistics code without the normalising sweep: one block, x and y unread.
template <bool TRAIN, bool SWEEP = true>
__global__ void __launch_bounds__(256) bn_normalize_kernel(const float* x, const float* __restrict__ mean, const float* __restrict__ m2_or_var,
                                                           int64_t rows, int dim, int rp, float eps, float momentum,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var, float* y,
                                                           float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  const int d4 = dim >> 2, t = threadIdx.x;
  if (t >= rp * d4) return;
  const int c = t % d4, rs = t / d4;
  const f32x4 mu = load4(mean + c * 4);
  const f32x4 m2 = load4(m2_or_var + c * 4);
  const f32x4 var = TRAIN ? m2 / (float)rows : m2;
  f32x4 rstd;
#pragma unroll
  for (int j = 0; j < 4; ++j) rstd[j] = rsqrtf(var[j] + eps);
  if (blockIdx.x == 0 && rs == 0) {
    if (mean_out) store4(mean_out + c * 4, mu);
    if (rstd_out) store4(rstd_out + c * 4, rstd);
    if (TRAIN && running_mean) {
      const float keep = 1.0f - momentum;
      store4(running_mean + c * 4, load4(running_mean + c * 4) * keep + mu * momentum);
      store4(running_var + c * 4, load4(running_var + c * 4) * keep + (m2 / (float)(rows - 1)) * momentum);
    }
  }
  if (!SWEEP) return;
  for (int64_t r = (int64_t)blockIdx.x * rp + rs; r < rows; r += (int64_t)gridDim.x * rp) {
    const int64_t o = r * dim + c * 4;
    store4(y + o, (load4(x + o) - mu) * rstd);
  }
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int64_t batchnorm_scratch_bytes(int64_t rows, int dim) {
  if (dim % 4 != 0 || dim < 4 || dim > 1024 || rows < 1 || rows >= ((int64_t)1 << 40) / dim) return -1;
  return ((int64_t)bn_geometry(rows, dim).grid + 3) * dim * (int64_t)sizeof(float);
}

// SWEEP = false: launch_batchnorm_stats, the statistics half (y is null and stays unread)
template <bool SWEEP>
static int batchnorm_impl(const float* x, int64_t rows, int dim, float eps, int training, float momentum, float* running_mean,
                          float* running_var, float* y, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  MAE_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= 1024, "batchnorm: dim %d must be a multiple of 4 in [4, 1024]", dim);
  MAE_REQUIRE(rows >= (training ? 2 : 1), "batchnorm: rows = %lld: training needs at least 2 rows, evaluation 1", (long long)rows);
  MAE_REQUIRE(rows < ((int64_t)1 << 40) / dim, "batchnorm: rows * dim = %lld * %d must stay below 2^40", (long long)rows, dim);
  MAE_REQUIRE(x && (y || !SWEEP), "batchnorm: x / y is null");
  MAE_REQUIRE(SWEEP || (mean_out && rstd_out), "batchnorm: the statistics call needs mean_out and rstd_out");
  MAE_REQUIRE(eps >= 0.f, "batchnorm: eps = %g must not be negative", (double)eps);
  MAE_REQUIRE((running_mean == nullptr) == (running_var == nullptr), "batchnorm: running_mean and running_var come together");
  MAE_REQUIRE(training || running_mean, "batchnorm: evaluation needs running_mean / running_var");
  MAE_REQUIRE(aligned16(x) && aligned16(y) && aligned16(running_mean) && aligned16(running_var) && aligned16(mean_out) && aligned16(rstd_out) &&
              aligned16(scratch), "batchnorm: every buffer must be 16-byte aligned");
  const int64_t bytes = rows * dim * (int64_t)sizeof(float);
  const char *xb = (const char*)x, *yb = (const char*)y;
  MAE_REQUIRE(!SWEEP || xb == yb || xb + bytes <= yb || yb + bytes <= xb, "batchnorm: y overlaps x partly (it may be x itself, or apart)");
  const BnGeo g = bn_geometry(rows, dim);
  const int ngrid = SWEEP ? (int)std::min<int64_t>(cdiv(rows, (int64_t)g.rp * BN_MIN_TRIPS), BN_NORM_BLOCKS) : 1;
  if (!training) {
    hipLaunchKernelGGL((bn_normalize_kernel<false, SWEEP>), dim3(ngrid), dim3(256), 0, s, x, running_mean, running_var, rows, dim, g.rp, eps, 0.f,
                       (float*)nullptr, (float*)nullptr, y, mean_out, rstd_out);
    MAE_LAUNCH_CHECK();
    return 0;
  }
  const int64_t need = batchnorm_scratch_bytes(rows, dim);
  MAE_REQUIRE(scratch && scratch_bytes >= need, "batchnorm: scratch_bytes = %lld, mae_batchnorm_scratch_bytes asks for %lld",
              (long long)scratch_bytes, (long long)need);
  MAE_REQUIRE(momentum >= 0.f && momentum <= 1.f, "batchnorm: momentum = %g outside [0, 1]", (double)momentum);
  float* partial = (float*)scratch;
  float* s0 = partial + (int64_t)g.grid * dim;
  float* m2 = s0 + dim;
  float* mean = m2 + dim;
  hipLaunchKernelGGL((bn_colsum_kernel<0>), dim3(g.grid), dim3(256), 0, s, x, (const float*)nullptr, rows, dim, g.rp, g.slice, (float*)nullptr, partial);
  MAE_LAUNCH_CHECK();
  MAE_TRY(launch_sum_partials(partial, g.grid, dim, s0, nullptr, dim, s));
  hipLaunchKernelGGL((bn_colsum_kernel<1>), dim3(g.grid), dim3(256), 0, s, x, (const float*)s0, rows, dim, g.rp, g.slice, mean, partial);
  MAE_LAUNCH_CHECK();
  MAE_TRY(launch_sum_partials(partial, g.grid, dim, m2, nullptr, dim, s));
  hipLaunchKernelGGL((bn_normalize_kernel<true, SWEEP>), dim3(ngrid), dim3(256), 0, s, x, (const float*)mean, (const float*)m2, rows, dim, g.rp, eps,
                     momentum, running_mean, running_var, y, mean_out, rstd_out);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_batchnorm_fwd(const float* x, int64_t rows, int dim, float eps, int training, float momentum, float* running_mean,
                         float* running_var, float* y, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  return batchnorm_impl<true>(x, rows, dim, eps, training, momentum, running_mean, running_var, y, mean_out, rstd_out, scratch, scratch_bytes, s);
}

int launch_batchnorm_stats(const float* x, int64_t rows, int dim, float eps, int training, float momentum, float* running_mean,
                           float* running_var, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  return batchnorm_impl<false>(x, rows, dim, eps, training, momentum, running_mean, running_var, nullptr, mean_out, rstd_out, scratch,
                               scratch_bytes, s);
}

// ---------------------------------------------------------------------------------------------------
// LARS: the two norms as sumsq_kernel forms them (block_sum_256 per block, a one-block finalize), then one sweep over p / g / mu;
// the device code is lars_dev.cuh, which mae_lars_step_groups (k_probe_sweep.hip) shares
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) lars_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t n4, float wd,
                                                         float* __restrict__ partial) {
  lars_sumsq_block(p, g, n4, wd, partial, blockIdx.x, gridDim.x);
}

__global__ void __launch_bounds__(256) lars_finalize_kernel(const float* __restrict__ partial, int nb, float trust, float* __restrict__ stats,
                                                            float* __restrict__ norms_out) {
  lars_finalize_block(partial, nb, trust, stats, norms_out);
}

template <bool ADAPT>
__global__ void __launch_bounds__(256) lars_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu, int64_t n4,
                                                          float lr, float momentum, float wd, const float* __restrict__ stats) {
  lars_update_block<ADAPT>(p, g, mu, n4, lr, momentum, wd, stats, blockIdx.x, gridDim.x);
}

int launch_lars_step(float* p, const float* g, float* mu, int64_t n, int adapt, float lr, float momentum, float wd, float trust,
                     float* norms_out, float* scratch, hipStream_t s) {
  MAE_REQUIRE(n >= 0 && n % 4 == 0, "lars: count = %lld must be a non-negative multiple of 4", (long long)n);
  if (n == 0) return 0;
  MAE_REQUIRE(p && g && mu && scratch, "lars: params / grads / mu / scratch is null");
  MAE_REQUIRE(aligned16(p) && aligned16(g) && aligned16(mu), "lars: params / grads / mu must be 16-byte aligned");
  const int64_t n4 = n / 4;
  if (adapt || norms_out) {
    const int grid = lars_sum_grid(n4);
    hipLaunchKernelGGL(lars_sumsq_kernel, dim3(grid), dim3(256), 0, s, p, g, n4, adapt ? wd : 0.f, scratch);
    MAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_finalize_kernel, dim3(1), dim3(256), 0, s, scratch, grid, trust, scratch + 2 * LARS_BLOCKS, norms_out);
    MAE_LAUNCH_CHECK();
  }
  const int grid = lars_update_grid(n4);
  with_bool(adapt != 0, [&](auto A) {  // without ADAPT the kernel reads neither wd nor the stats
    hipLaunchKernelGGL((lars_update_kernel<decltype(A)::value>), dim3(grid), dim3(256), 0, s, p, g, mu, n4, lr, momentum, wd, scratch + 2 * LARS_BLOCKS);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int64_t mae_batchnorm_scratch_bytes(int64_t rows, int32_t dim) { return mae::batchnorm_scratch_bytes(rows, dim); }

extern "C" int mae_batchnorm_fwd(const float* x, int64_t rows, int32_t dim, float eps, int32_t training, float momentum, float* running_mean,
                                 float* running_var, float* y, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  return mae::launch_batchnorm_fwd(x, rows, dim, eps, training, momentum, running_mean, running_var, y, mean_out, rstd_out, scratch,
                                   scratch_bytes, (hipStream_t)stream);
}

extern "C" int mae_batchnorm_stats(const float* x, int64_t rows, int32_t dim, float eps, int32_t training, float momentum, float* running_mean,
                                   float* running_var, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, void* stream) {
  return mae::launch_batchnorm_stats(x, rows, dim, eps, training, momentum, running_mean, running_var, mean_out, rstd_out, scratch,
                                     scratch_bytes, (hipStream_t)stream);
}

extern "C" int mae_lars_step(float* params, const float* grads, float* mu, int64_t count, int32_t adapt, float lr, float momentum,
                             float weight_decay, float trust_coefficient, float* norms_out, float* scratch, void* stream) {
  return mae::launch_lars_step(params, grads, mu, count, adapt, lr, momentum, weight_decay, trust_coefficient, norms_out, scratch,
                               (hipStream_t)stream);
}
