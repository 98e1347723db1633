// Normalised-pixel targets (the MAE paper's norm_pix_loss; no counterpart in the reference, whose target is the raw patch,
// src/models/mae.py:90-92): every masked patch x (P = p*p*C values in (py, px, c) order, what mae_patchify_gather returns) is
// standardised by its own statistics,
//     mean = sum(x) / P,  var = sum((x - mean)^2) / (P - 1),  t = (x - mean) / sqrt(var + MAE_NORM_PIX_EPS).
// Three kernels share one walk: the fused loss (target never written), the materialising gather and the inverse.
//
// Walk: one WAVE per masked token, four per workgroup.  The wave copies its patch from the image (uint8 pixels go through
// norm_u8 first, so both image formats give the same floats from here on) into its own P floats of LDS, reading in image
// order (runs of p contiguous pixels) and writing in output order.  Statistics: lanes stride over the P values, a wave
// butterfly adds the 64 partial sums; the order depends on P alone, so a row comes out bit-identical from run to run, in
// any batch and from either image format.  The mean is taken about the patch's first value (mean = x0 + sum(x - x0) / P):
// a constant patch then has mean == x0, centred values and variance exactly 0 and t == 0 exactly, whatever P is.  The
// variance is two-pass (centre, then square): E[x^2] - E[x]^2 would lose every digit on flat uint8 regions, exactly where
// rstd is ~1000.
#include "kernels.h"

namespace mae {

namespace {

constexpr int NP_WAVES = 4;   // waves (= tokens in flight) per workgroup of 256

// 1 / sqrt(v), v > 0, to within an ulp: IEEE sqrt and division, then one Newton step on the residual 1 - v r^2 formed without
// rounding (the product v r is split into head and tail).  v = fp32(1e-6) gives exactly 1000.
__device__ __forceinline__ float rsqrt_refined(float v) {
  const float r = __fdiv_rn(1.0f, __fsqrt_rn(v));
  const float h = __fmul_rn(v, r), hl = fmaf(v, r, -h);
  float e = fmaf(-h, r, 1.0f);
  e = fmaf(-hl, r, e);
  return fmaf(0.5f * r, e, r);
}

// token id of row r (int64 on the API, int32 inside the engine) -> patch number clamped into the grid, as mae_patchify_gather does
__device__ __forceinline__ int row_patch(const void* idx, int idx64, int64_t r, int g) {
  const int64_t t = idx64 ? static_cast<const int64_t*>(idx)[r] : (int64_t) static_cast<const int32_t*>(idx)[r];
  const int64_t n = t - 1;
  return n < 0 ? 0 : (n >= (int64_t)g * g ? g * g - 1 : (int)n);
}

// one wave: patch n of image b -> wl[P] in (py, px, c) order
template <class IMG>
__device__ __forceinline__ void load_patch(const IMG* __restrict__ images, int64_t b, int n, int C, int img, int p, float* wl) {
  const int g = img / p, pp = p * p, lane = threadIdx.x & 63;
  const int ph = n / g, pw = n - ph * g;
  const IMG* base = images + (b * C * (int64_t)img + ph * p) * img + pw * p;
  for (int i = lane; i < C * pp; i += 64) {
    const int c = i / pp, q = i - c * pp;
    const int py = q / p, px = q - py * p;
    wl[q * C + c] = px_value(base + ((int64_t)c * img + py) * img + px);
  }
}

// one wave, after the patch is visible in wl: mean and variance (every lane gets the same bits)
__device__ __forceinline__ void patch_stats(const float* wl, int P, float& mean, float& var) {
  const int lane = threadIdx.x & 63;
  const float x0 = wl[0];
  float s = 0.f;
  for (int i = lane; i < P; i += 64) s += wl[i] - x0;
  mean = x0 + __fdiv_rn(wave_sum(s), (float)P);
  float q = 0.f;
  for (int i = lane; i < P; i += 64) {
    const float d = wl[i] - mean;
    q = fmaf(d, d, q);
  }
  var = __fdiv_rn(wave_sum(q), (float)(P - 1));
}

// the one expression of the target: both roundings spelled out so that the fused loss and the materialised target agree bit for bit
__device__ __forceinline__ float standardise(float x, float mean, float rstd) { return __fmul_rn(__fsub_rn(x, mean), rstd); }

// Every kernel below: rows = B * m tokens, workgroup w takes rows 4w .. 4w+3, then strides by 4 * gridDim; the trip count is the
// same for the four waves of a workgroup (the barriers sit outside the `on` branches).

template <class IMG, class T, bool HAS_GRAD>
__global__ void __launch_bounds__(256) mse_norm_pix_kernel(const float* __restrict__ pred, const IMG* __restrict__ images, const void* __restrict__ idx,
                                                           int idx64, int64_t rows, int m, int C, int img, int p, float gscale,
                                                           float* __restrict__ partial, T* __restrict__ dpred) {
  extern __shared__ __attribute__((aligned(16))) float np_lds[];
  __shared__ float red[4];
  const int P = C * p * p, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wl = np_lds + w * P;
  float acc = 0.f;
  for (int64_t r0 = (int64_t)blockIdx.x * NP_WAVES; r0 < rows; r0 += (int64_t)gridDim.x * NP_WAVES) {
    const int64_t r = r0 + w;
    const bool on = r < rows;
    if (on) load_patch(images, r / m, row_patch(idx, idx64, r, img / p), C, img, p, wl);
    __syncthreads();
    if (on) {
      float mean, var;
      patch_stats(wl, P, mean, var);
      const float rstd = rsqrt_refined(var + (float)MAE_NORM_PIX_EPS);
      const float* pr = pred + r * P;
      for (int i = lane; i < P; i += 64) {
        const float d = pr[i] - standardise(wl[i], mean, rstd);
        acc = fmaf(d, d, acc);
        if (HAS_GRAD) dpred[r * P + i] = from_f<T>(d * gscale);
      }
    }
    __syncthreads();
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <class IMG>
__global__ void __launch_bounds__(256) patchify_norm_kernel(const IMG* __restrict__ images, const void* __restrict__ idx, int idx64, int64_t rows,
                                                            int m, int C, int img, int p, float* __restrict__ target,
                                                            float* __restrict__ mean_out, float* __restrict__ rstd_out) {
  extern __shared__ __attribute__((aligned(16))) float np_lds[];
  const int P = C * p * p, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wl = np_lds + w * P;
  for (int64_t r0 = (int64_t)blockIdx.x * NP_WAVES; r0 < rows; r0 += (int64_t)gridDim.x * NP_WAVES) {
    const int64_t r = r0 + w;
    const bool on = r < rows;
    if (on) load_patch(images, r / m, row_patch(idx, idx64, r, img / p), C, img, p, wl);
    __syncthreads();
    if (on) {
      float mean, var;
      patch_stats(wl, P, mean, var);
      const float rstd = rsqrt_refined(var + (float)MAE_NORM_PIX_EPS);
      for (int i = lane; i < P; i += 64) target[r * P + i] = standardise(wl[i], mean, rstd);
      if (lane == 0) {
        if (mean_out) mean_out[r] = mean;
        if (rstd_out) rstd_out[r] = rstd;
      }
    }
    __syncthreads();
  }
}

// out = pred * sqrt(var + eps) + mean; out may be pred (each element is read and written by the same lane)
template <class IMG>
__global__ void __launch_bounds__(256) norm_pix_restore_kernel(const IMG* __restrict__ images, const float* pred, const void* __restrict__ idx,
                                                               int idx64, int64_t rows, int m, int C, int img, int p, float* out) {
  extern __shared__ __attribute__((aligned(16))) float np_lds[];
  const int P = C * p * p, w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float* wl = np_lds + w * P;
  for (int64_t r0 = (int64_t)blockIdx.x * NP_WAVES; r0 < rows; r0 += (int64_t)gridDim.x * NP_WAVES) {
    const int64_t r = r0 + w;
    const bool on = r < rows;
    if (on) load_patch(images, r / m, row_patch(idx, idx64, r, img / p), C, img, p, wl);
    __syncthreads();
    if (on) {
      float mean, var;
      patch_stats(wl, P, mean, var);
      const float sd = __fsqrt_rn(var + (float)MAE_NORM_PIX_EPS);
      for (int i = lane; i < P; i += 64) out[r * P + i] = fmaf(pred[r * P + i], sd, mean);
    }
    __syncthreads();
  }
}

constexpr size_t NP_LDS_MAX = 160 * 1024 - 64;   // the CU's LDS less the kernels' static reduction buffer; four patches must fit (P <= 10236)

int check_geometry(const char* who, const void* images, int img_dt, const void* idx, int B, int m, int C, int img, int p) {
  MAE_REQUIRE(images && idx && B > 0 && m > 0 && C > 0, "%s: bad arguments", who);
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "%s: image dtype must be MAE_F32 or MAE_U8", who);
  MAE_REQUIRE(p > 0 && img > 0 && img % p == 0, "%s: image_size %d must be a positive multiple of patch_size %d", who, img, p);
  MAE_REQUIRE((int64_t)C * p * p >= 2, "%s: a patch of one value has no variance", who);
  MAE_REQUIRE((size_t)C * p * p * 4 * NP_WAVES <= NP_LDS_MAX, "%s: patch_size^2 * in_chans = %lld exceeds %d values", who,
              (long long)C * p * p, (int)(NP_LDS_MAX / (4 * NP_WAVES)));
  MAE_REQUIRE((int64_t)(img / p) * (img / p) < (1ll << 31), "%s: too many patches", who);
  if (img_dt == MAE_F32) MAE_REQUIRE(((uintptr_t)images & 3) == 0, "%s: fp32 images must be 4-byte aligned", who);
  return 0;
}

}  // namespace

int launch_mse_norm_pix(const float* pred, const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p,
                        float grad_scale, float* loss, void* d_pred, int dpred_dt, float* scratch, hipStream_t s) {
  MAE_TRY(check_geometry("mse_norm_pix", images, img_dt, idx, B, m, C, img, p));
  MAE_REQUIRE(pred && loss && scratch, "mse_norm_pix: null pred/loss/scratch");
  MAE_REQUIRE(!d_pred || dpred_dt == MAE_F32 || dpred_dt == MAE_BF16, "mse_norm_pix: d_pred dtype must be MAE_F32 or MAE_BF16");
  MAE_REQUIRE((((uintptr_t)pred | (uintptr_t)loss | (uintptr_t)scratch) & 3) == 0 && ((uintptr_t)d_pred & (dpred_dt == MAE_BF16 ? 1 : 3)) == 0,
              "mse_norm_pix: misaligned buffer");
  const int64_t rows = (int64_t)B * m, n = rows * p * p * C;
  const int grid = (int)std::min<int64_t>(cdiv(rows, NP_WAVES), RED_BLOCKS);
  const float gs = grad_scale * 2.0f / (float)n;
  const size_t lds = (size_t)C * p * p * 4 * NP_WAVES;
  if (img_dt == MAE_U8)
    MAE_LAUNCH_LOSS(mse_norm_pix_kernel, (uint8_t,), grid, lds, s, d_pred, dpred_dt, scratch, 1.0f / (float)n, loss, pred, (const uint8_t*)images, idx, idx64,
                    rows, m, C, img, p, gs);
  else
    MAE_LAUNCH_LOSS(mse_norm_pix_kernel, (float,), grid, lds, s, d_pred, dpred_dt, scratch, 1.0f / (float)n, loss, pred, (const float*)images, idx, idx64,
                    rows, m, C, img, p, gs);
  return 0;
}

int launch_patchify_gather_norm(const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p, float* target,
                                float* mean, float* rstd, hipStream_t s) {
  MAE_TRY(check_geometry("patchify_gather_norm", images, img_dt, idx, B, m, C, img, p));
  MAE_REQUIRE(target && (((uintptr_t)target | (uintptr_t)mean | (uintptr_t)rstd) & 3) == 0, "patchify_gather_norm: null or misaligned output");
  const int64_t rows = (int64_t)B * m;
  const int grid = (int)std::min<int64_t>(cdiv(rows, NP_WAVES), 256 * 16);
  const size_t lds = (size_t)C * p * p * 4 * NP_WAVES;
  if (img_dt == MAE_U8) {
    MAE_TRY(allow_lds(patchify_norm_kernel<uint8_t>, lds));
    hipLaunchKernelGGL((patchify_norm_kernel<uint8_t>), dim3(grid), dim3(256), lds, s, (const uint8_t*)images, idx, idx64, rows, m, C, img, p, target, mean, rstd);
  } else {
    MAE_TRY(allow_lds(patchify_norm_kernel<float>, lds));
    hipLaunchKernelGGL((patchify_norm_kernel<float>), dim3(grid), dim3(256), lds, s, (const float*)images, idx, idx64, rows, m, C, img, p, target, mean, rstd);
  }
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_norm_pix_restore(const void* images, int img_dt, const float* pred, const void* idx, int idx64, int B, int m, int C, int img, int p,
                            float* out, hipStream_t s) {
  MAE_TRY(check_geometry("norm_pix_restore", images, img_dt, idx, B, m, C, img, p));
  MAE_REQUIRE(pred && out && (((uintptr_t)pred | (uintptr_t)out) & 3) == 0, "norm_pix_restore: null or misaligned pred/out");
  const int64_t rows = (int64_t)B * m, bytes = rows * C * p * p * 4;
  const uintptr_t a = (uintptr_t)pred, o = (uintptr_t)out;
  MAE_REQUIRE(a == o || a + bytes <= o || o + bytes <= a, "norm_pix_restore: out may be pred itself but not overlap it partially");
  const int grid = (int)std::min<int64_t>(cdiv(rows, NP_WAVES), 256 * 16);
  const size_t lds = (size_t)C * p * p * 4 * NP_WAVES;
  if (img_dt == MAE_U8) {
    MAE_TRY(allow_lds(norm_pix_restore_kernel<uint8_t>, lds));
    hipLaunchKernelGGL((norm_pix_restore_kernel<uint8_t>), dim3(grid), dim3(256), lds, s, (const uint8_t*)images, pred, idx, idx64, rows, m, C, img, p, out);
  } else {
    MAE_TRY(allow_lds(norm_pix_restore_kernel<float>, lds));
    hipLaunchKernelGGL((norm_pix_restore_kernel<float>), dim3(grid), dim3(256), lds, s, (const float*)images, pred, idx, idx64, rows, m, C, img, p, out);
  }
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_patchify_gather_norm(const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch, int32_t in_chans,
                                        int32_t image_size, int32_t patch_size, int32_t num_mask, float* target, float* mean, float* rstd,
                                        void* stream) {
  return mae::launch_patchify_gather_norm(images, image_dtype, idx_mask, 1, batch, num_mask, in_chans, image_size, patch_size, target, mean, rstd,
                                          (hipStream_t)stream);
}

extern "C" int mae_mse_loss_norm_pix(const float* pred, const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch,
                                     int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float grad_scale, float* loss,
                                     void* d_pred, int32_t d_pred_dtype, float* scratch, void* stream) {
  return mae::launch_mse_norm_pix(pred, images, image_dtype, idx_mask, 1, batch, num_mask, in_chans, image_size, patch_size, grad_scale, loss,
                                  d_pred, d_pred_dtype, scratch, (hipStream_t)stream);
}

extern "C" int mae_norm_pix_restore(const void* images, int32_t image_dtype, const float* pred, const int64_t* idx_mask, int32_t batch,
                                    int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float* out, void* stream) {
  return mae::launch_norm_pix_restore(images, image_dtype, pred, idx_mask, 1, batch, num_mask, in_chans, image_size, patch_size, out,
                                      (hipStream_t)stream);
}
