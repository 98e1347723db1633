// LayerNorm(eps) forward / backward over fp32 residual-stream rows; LPR lanes per row (64, 32 or 16: a wave walks 1, 2 or 4
// rows at a time so that 384- and 192-wide rows = 96 / 48 float4 fill every lane; at 64 lanes per row a quarter of the lanes
// idled), the row held in registers, mean/variance by shuffles inside the lane group.  HBM-bound: fwd reads 4*D B/row,
// writes sizeof(T)*D.  Cache policy as measured on the step: store4_nt for the fp32 residual-stream and dx stores (-0.4 ms), load4_nt
// for the read-once x, branch and dy (-0.2 ms, mostly in the GEMMs that follow), plain store4 for the y / dx_copy copies (no gain).
// Reference behaviour: torch.nn.LayerNorm(dim, eps=1e-6) as timm VisionTransformer / lightly MAEDecoderTIMM
// instantiate it (norm1/norm2/norm/decoder_norm), computed in fp32 (autocast keeps layer_norm in fp32).
#include "kernels.h"

namespace mae {

template <int LPR>
__device__ __forceinline__ float group_sum(float v) {  // sum over the LPR consecutive lanes that share a row
#pragma unroll
  for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// lanes per row for a row of d4 float4: the widest group that wastes no more lanes than a narrower one would
static int ln_lanes_per_row(int d4) {
  int best = 64;
  double best_fill = (double)d4 / (64.0 * (double)cdiv(d4, 64));
  for (int lpr : {32, 16}) {
    if (cdiv(d4, lpr) > 4) continue;
    const double fill = (double)d4 / ((double)lpr * (double)cdiv(d4, lpr));
    if (fill > best_fill + 1e-9) { best_fill = fill; best = lpr; }
  }
  return best;
}
// The eight (lanes per row, float4 per lane) pairs that ln_lanes_per_row gives for dim 4..1024, and the only ones compiled:
// f(integral_constant<LPR>, integral_constant<NV>) for the pair (lpr, nv)
template <int N> using int_c = std::integral_constant<int, N>;
template <class F>
static int with_ln_shape(int lpr, int nv, F&& f) {
  switch (lpr * 8 + nv) {
    case 16 * 8 + 1: f(int_c<16>{}, int_c<1>{}); break;
    case 32 * 8 + 1: f(int_c<32>{}, int_c<1>{}); break;
    case 16 * 8 + 3: f(int_c<16>{}, int_c<3>{}); break;
    case 64 * 8 + 1: f(int_c<64>{}, int_c<1>{}); break;
    case 32 * 8 + 3: f(int_c<32>{}, int_c<3>{}); break;
    case 64 * 8 + 2: f(int_c<64>{}, int_c<2>{}); break;
    case 64 * 8 + 3: f(int_c<64>{}, int_c<3>{}); break;
    case 64 * 8 + 4: f(int_c<64>{}, int_c<4>{}); break;
    default: MAE_REQUIRE(false, "layernorm: no kernel for lpr = %d lanes per row with nv = %d float4 per lane", lpr, nv);
  }
  return 0;
}

// NV = float4 vectors per lane: covers dim <= 4*LPR*NV
// ADD: the LayerNorm input is x + branch (the residual add of the preceding attention / MLP branch, whose GEMM then
// keeps the plain bf16 epilogue); the sum is written to x_out as the new fp32 residual stream.
// SCALE (with ADD; drop path): instantiated with the trailing arguments (const float* image_scale, int
// rows_per_image), the branch of full-matrix row src is multiplied by image_scale[src / rows_per_image] in fp32 before the add.  A
// scale of exactly 0 skips the branch load: x_out is then x bit for bit whatever the branch rows hold.  The lane groups of a wave can
// belong to images with different scales, so only the loads and the add sit under the test on the scale; the group_sum shuffles
// stay outside it.  Without the trailing arguments (the empty pack) the kernel has the signature and the code it had before.
__device__ __forceinline__ const float* ln_scale_ptr() { return nullptr; }
__device__ __forceinline__ const float* ln_scale_ptr(const float* p, int) { return p; }
__device__ __forceinline__ int ln_scale_rows() { return 1; }
__device__ __forceinline__ int ln_scale_rows(const float*, int rows_per_image) { return rows_per_image; }

template <class T, int NV, bool ADD, int LPR, class... S>
__global__ void __launch_bounds__(256) layernorm_fwd_kernel(const float* __restrict__ x, const T* __restrict__ branch,
                                                            float* __restrict__ x_out, const int32_t* __restrict__ row_map,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            float eps, int64_t rows, int dim, T* __restrict__ y,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out, S... scale_args) {
  constexpr bool SCALE = sizeof...(S) != 0;
  static_assert(ADD || !SCALE, "an image scale needs the fused add");
  constexpr int RPW = 64 / LPR;  // rows per wave and iteration
  const int lane = threadIdx.x & 63, li = lane & (LPR - 1), sub = lane / LPR;
  const int D4 = dim >> 2;
  const float inv_d = 1.0f / (float)dim;
  for (int64_t r0 = (blockIdx.x * 4ll + (threadIdx.x >> 6)) * RPW; r0 < rows; r0 += (int64_t)gridDim.x * 4 * RPW) {
    const bool live = r0 + sub < rows;                 // lane groups past the last row compute on it and store nothing
    const int64_t r = live ? r0 + sub : rows - 1;
    const int64_t src = row_map ? (int64_t)row_map[r] : r;
    const float* px = x + src * dim;
    float sc = 1.f;
    if (SCALE) sc = ln_scale_ptr(scale_args...)[src / ln_scale_rows(scale_args...)];  // lane groups past the last row: row rows - 1 and its scale
    f32x4 v[NV];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = li + LPR * i;
      if (c < D4) {
        v[i] = load4_nt(px + c * 4);
        if (ADD) {
          if (!SCALE) v[i] += load4_nt(branch + src * dim + c * 4);
          else if (sc != 0.f) v[i] += load4_nt(branch + src * dim + c * 4) * sc;
          if (live) store4_nt(x_out + src * dim + c * 4, v[i]);
        }
        sum += v[i][0] + v[i][1] + v[i][2] + v[i][3];
      } else {
        v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    const float mean = group_sum<LPR>(sum) * inv_d;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = li + LPR * i;
      if (c < D4) {
        const f32x4 d = v[i] - mean;
        sq += sumsq4(d);
      }
    }
    const float var = group_sum<LPR>(sq) * inv_d;
    const float rstd = rsqrtf(var + eps);
    T* py = y + r * dim;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = li + LPR * i;
      if (c < D4 && live) {
        const f32x4 o = (v[i] - mean) * rstd * load4(gamma + c * 4) + load4(beta + c * 4);
        store4(py + c * 4, o);
      }
    }
    if (li == 0 && live) {
      mean_out[r] = mean;
      rstd_out[r] = rstd;
    }
  }
}

// image_scale (NULL: none, the launches of before): the drop-path scale per image of the fused add; src / rows_per_image indexes it.
int launch_layernorm_fwd(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                         const float* beta, float eps, int64_t rows, int dim, int y_dt, void* y, float* mean, float* rstd,
                         hipStream_t s, const float* image_scale, int rows_per_image) {
  MAE_REQUIRE(x && gamma && beta && y && mean && rstd && rows > 0, "layernorm_fwd: null buffer");
  MAE_REQUIRE(!branch || x_out, "layernorm_fwd: the fused residual add needs x_out");
  MAE_REQUIRE(!image_scale || (branch && rows_per_image > 0), "layernorm_fwd: an image scale needs a branch and rows_per_image > 0");
  MAE_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= 1024, "layernorm: dim %d must be a multiple of 4 in [4, 1024]", dim);
  const int lpr = ln_lanes_per_row(dim / 4), nv = (int)cdiv(dim / 4, lpr);
  const int grid = (int)std::min<int64_t>(cdiv(rows, 4 * (64 / lpr)), 256 * 32);
  const auto launch = [&](auto add, auto... scale) {  // scale: () or (image_scale, rows_per_image)
    int rc = 0;
    with_dtype(y_dt, [&](auto t) {
      using T = decltype(t);
      rc = with_ln_shape(lpr, nv, [&](auto L, auto N) {
        hipLaunchKernelGGL((layernorm_fwd_kernel<T, decltype(N)::value, decltype(add)::value, decltype(L)::value, decltype(scale)...>), dim3(grid),
                           dim3(256), 0, s, x, (const T*)branch, x_out, row_map, gamma, beta, eps, rows, dim, (T*)y, mean, rstd, scale...);
      });
    });
    return rc;
  };
  if (image_scale) MAE_TRY(launch(std::true_type{}, image_scale, rows_per_image));
  else if (branch) MAE_TRY(launch(std::true_type{}));
  else MAE_TRY(launch(std::false_type{}));
  MAE_LAUNCH_CHECK();
  return 0;
}

// Backward.  xhat = (x-mean)*rstd, g = dy*gamma:
//   dx = rstd * (g - mean(g) - xhat*mean(g*xhat));  dgamma = sum_rows dy*xhat;  dbeta = sum_rows dy
// Each wave keeps per-lane column partials of dgamma/dbeta across the rows it walks; the block's 4 waves are
// combined through LDS into partial[block][2][dim]; a second kernel adds the blocks in order (deterministic).
// SCALE (drop path; the trailing arguments const float* copy_scale, int rows_per_image): dx_copy[src] =
// T(fl32(copy_scale[src / rows_per_image] * d)), d the fp32 value stored to dx_io[src]: the copy is the gradient entering the branch
// that reads it next.  dx_io, dgamma and dbeta do not see the scale.  Without the trailing arguments: the kernel as it was.
template <class T, int NV, int LPR, class... S>
__global__ void __launch_bounds__(256) layernorm_bwd_kernel(const T* __restrict__ dy, const float* __restrict__ x,
                                                            const int32_t* __restrict__ row_map,
                                                            const float* __restrict__ gamma, const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, int64_t rows, int dim,
                                                            int accumulate, float* __restrict__ dx_io, T* __restrict__ dx_copy,
                                                            float* __restrict__ partial, S... scale_args) {
  constexpr bool SCALE = sizeof...(S) != 0;
  constexpr int RPW = 64 / LPR;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves x RPW lane groups][2][dim]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & (LPR - 1), sub = lane / LPR;
  const int D4 = dim >> 2;
  const float inv_d = 1.0f / (float)dim;
  f32x4 gam[NV], dg[NV], db[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = li + LPR * i;
    gam[i] = (c < D4) ? load4(gamma + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    dg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    db[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int64_t r0 = (blockIdx.x * 4ll + wave) * RPW; r0 < rows; r0 += (int64_t)gridDim.x * 4 * RPW) {
    const bool live = r0 + sub < rows;
    const int64_t r = live ? r0 + sub : rows - 1;
    const int64_t src = row_map ? (int64_t)row_map[r] : r;
    const float mu = mean[r], rs = rstd[r];
    float sc = 1.f;
    if (SCALE) sc = ln_scale_ptr(scale_args...)[src / ln_scale_rows(scale_args...)];
    f32x4 xh[NV], g[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = li + LPR * i;
      if (c < D4) {
        const f32x4 d = load4_nt(dy + r * dim + c * 4);
        xh[i] = (load4_nt(x + src * dim + c * 4) - mu) * rs;
        g[i] = d * gam[i];
        if (live) {
          dg[i] += d * xh[i];
          db[i] += d;
        }
        s1 += g[i][0] + g[i][1] + g[i][2] + g[i][3];
        s2 += g[i][0] * xh[i][0] + g[i][1] * xh[i][1] + g[i][2] * xh[i][2] + g[i][3] * xh[i][3];
      }
    }
    s1 = group_sum<LPR>(s1) * inv_d;
    s2 = group_sum<LPR>(s2) * inv_d;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = li + LPR * i;
      if (c < D4 && live) {
        f32x4 d = (g[i] - s1 - xh[i] * s2) * rs;
        float* pd = dx_io + src * dim + c * 4;
        if (accumulate) d += load4(pd);
        store4_nt(pd, d);
        if (SCALE) store4(dx_copy + src * dim + c * 4, d * sc);
        else if (dx_copy) store4(dx_copy + src * dim + c * 4, d);
      }
    }
  }
  // block reduce of the column partials: 4 * RPW lane groups hold partials of the same columns
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = li + LPR * i;
    if (c < D4) {
      store4(red + ((wave * RPW + sub) * 2 + 0) * dim + c * 4, dg[i]);
      store4(red + ((wave * RPW + sub) * 2 + 1) * dim + c * 4, db[i]);
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * dim; c += 256) {
    float v = 0.f;
#pragma unroll
    for (int gidx = 0; gidx < 4 * RPW; ++gidx) v += red[gidx * 2 * dim + c];
    partial[(int64_t)blockIdx.x * 2 * dim + c] = v;
  }
}

int launch_layernorm_bwd(const void* dy, int dy_dt, const float* x, const int32_t* row_map, const float* gamma,
                         const float* mean, const float* rstd, int64_t rows, int dim, int accumulate, float* dx_io,
                         void* dx_copy, float* dgamma, float* dbeta, float* partial, hipStream_t s, PartialsTable* defer,
                         const float* copy_scale, int rows_per_image) {
  MAE_REQUIRE(dy && x && gamma && mean && rstd && dx_io && dgamma && dbeta && partial && rows > 0, "layernorm_bwd: null buffer");
  MAE_REQUIRE(!copy_scale || (dx_copy && rows_per_image > 0), "layernorm_bwd: a copy scale needs dx_copy and rows_per_image > 0");
  MAE_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= 1024, "layernorm: dim %d must be a multiple of 4 in [4, 1024]", dim);
  if (defer && defer->n == PartialsTable::MAX) {  // deep models: run what is queued before `partial` (slot 0 again) is rewritten
    MAE_TRY(launch_sum_partials_many(*defer, s));
    defer->n = 0;
  }
  const int lpr = ln_lanes_per_row(dim / 4), nv = (int)cdiv(dim / 4, lpr);
  const int grid = (int)std::min<int64_t>(cdiv(rows, 4 * (64 / lpr)), LN_BWD_MAX_BLOCKS);
  const size_t lds = (size_t)8 * (64 / lpr) * dim * sizeof(float);
  const auto launch = [&](auto... scale) {  // scale: () or (copy_scale, rows_per_image)
    int rc = 0;
    with_dtype(dy_dt, [&](auto t) {
      using T = decltype(t);
      rc = with_ln_shape(lpr, nv, [&](auto L, auto N) {
        hipLaunchKernelGGL((layernorm_bwd_kernel<T, decltype(N)::value, decltype(L)::value, decltype(scale)...>), dim3(grid), dim3(256), lds, s,
                           (const T*)dy, x, row_map, gamma, mean, rstd, rows, dim, accumulate, dx_io, (T*)dx_copy, partial, scale...);
      });
    });
    return rc;
  };
  MAE_TRY(copy_scale ? launch(copy_scale, rows_per_image) : launch());
  MAE_LAUNCH_CHECK();
  if (defer) {
    const int i = defer->n++;
    if (i == 0) defer->block_begin[0] = 0;
    defer->partial[i] = partial; defer->out0[i] = dgamma; defer->out1[i] = dbeta;
    defer->G[i] = grid; defer->C[i] = 2 * dim; defer->split[i] = dim;
    defer->block_begin[i + 1] = defer->block_begin[i] + (int)cdiv(2 * dim, 32);
    return 0;
  }
  return launch_sum_partials(partial, grid, 2 * dim, dgamma, dbeta, dim, s);
}

}  // namespace mae

extern "C" int mae_layernorm_fwd(const float* x, const int32_t* row_map, const float* gamma, const float* beta, float eps,
                                 int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean, float* rstd,
                                 void* stream) {
  return mae::launch_layernorm_fwd(x, nullptr, nullptr, row_map, gamma, beta, eps, rows, dim, y_dtype, y, mean, rstd, (hipStream_t)stream);
}

extern "C" int mae_add_layernorm_fwd(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                                     const float* beta, float eps, int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean,
                                     float* rstd, void* stream) {
  MAE_REQUIRE(branch && x_out, "mae_add_layernorm_fwd: null branch/x_out");
  return mae::launch_layernorm_fwd(x, branch, x_out, row_map, gamma, beta, eps, rows, dim, y_dtype, y, mean, rstd, (hipStream_t)stream);
}

extern "C" int mae_layernorm_bwd(const void* dy, int32_t dy_dtype, const float* x, const int32_t* row_map,
                                 const float* gamma, const float* mean, const float* rstd, int64_t rows, int32_t dim,
                                 int32_t accumulate, float* dx_io, void* dx_copy, float* dgamma, float* dbeta,
                                 float* partial, void* stream) {
  return mae::launch_layernorm_bwd(dy, dy_dtype, x, row_map, gamma, mean, rstd, rows, dim, accumulate, dx_io, dx_copy,
                                   dgamma, dbeta, partial, (hipStream_t)stream);
}

extern "C" int mae_add_layernorm_fwd_scaled(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                                            const float* beta, float eps, int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean,
                                            float* rstd, const float* image_scale, int32_t rows_per_image, void* stream) {
  MAE_REQUIRE(branch && x_out, "mae_add_layernorm_fwd_scaled: null branch/x_out");
  MAE_REQUIRE(rows_per_image > 0, "mae_add_layernorm_fwd_scaled: rows_per_image = %d must be positive", rows_per_image);
  return mae::launch_layernorm_fwd(x, branch, x_out, row_map, gamma, beta, eps, rows, dim, y_dtype, y, mean, rstd, (hipStream_t)stream,
                                   image_scale, rows_per_image);
}

extern "C" int mae_layernorm_bwd_scaled(const void* dy, int32_t dy_dtype, const float* x, const int32_t* row_map,
                                        const float* gamma, const float* mean, const float* rstd, int64_t rows, int32_t dim,
                                        int32_t accumulate, float* dx_io, void* dx_copy, float* dgamma, float* dbeta,
                                        float* partial, const float* copy_scale, int32_t rows_per_image, void* stream) {
  MAE_REQUIRE(rows_per_image > 0, "mae_layernorm_bwd_scaled: rows_per_image = %d must be positive", rows_per_image);
  MAE_REQUIRE(!copy_scale || dx_copy, "mae_layernorm_bwd_scaled: a copy scale needs dx_copy");
  return mae::launch_layernorm_bwd(dy, dy_dtype, x, row_map, gamma, mean, rstd, rows, dim, accumulate, dx_io, dx_copy,
                                   dgamma, dbeta, partial, (hipStream_t)stream, nullptr, copy_scale, rows_per_image);
}
