// The three kernel families that read the image: visible-patch gather (im2col of the kept patches only), masked-pixel MSE against
// the image (target never materialised) and target patchify-gather.  Images are normalised fp32 or uint8; uint8 pixels get
// ToTensor + Normalize(.5, .5) fused into the read (reference: src/data.py:15-24 builds transforms.ToTensor() -> x / 255, then
// Normalize(mean .5, std .5) -> (x - .5) / .5; here v = (u8 / 255 - 0.5) / 0.5 with an IEEE-rounded division, bit-identical to the
// torch fp32 expression).  Reference behaviour:
//   gather_patches + patch GEMM + assemble_visible == timm PatchEmbed conv (k = s = patch) -> cat(cls) -> +pos_embed
//     -> gather(idx_keep)           (lightly MaskedVisionTransformerTIMM.preprocess, via src/models/mae.py:55)
//   patchify_gather == utils.patchify + get_at_index(clamp(idx_mask-1, 0))   (src/models/mae.py:90-92)
//   mse_from_images == torch.nn.MSELoss() of the prediction against that target (src/training/mae.py:40,48)
//
// Two ways to move the data.  The per-pixel gathers (float images; any patch size, any alignment) read patch rows where they lie.
// The BAND WALK (every uint8 reader, and the float loss where the geometry allows): a patch row of a uint8 image is p bytes (8 for
// ViT-S/8), far below a 128-byte HBM line, so a gather by patch would pull 16x the bytes it uses.  Instead one workgroup owns one
// BAND = one row of patches of one image (C x p x W pixels: 2.3 KB of uint8 at 96 px / p 8, 10.5 KB at 224 px / p 16), streams it
// into LDS with coalesced loads, then serves the band's visible (or masked) tokens from LDS.  Every image byte is fetched exactly
// once per kernel: 27.6 KB per uint8 image instead of the 110.6 KB fp32 image read as scattered 32-byte patch rows (3.9x / 2.3x
// over-fetch measured in round 1); the float loss's gather pulled 759 MB for 221 MB of pixels at batch 2000 (PMC round 3).
// All HBM-bound, 55 MB per launch at batch 2000 with uint8 images.
#include "kernels.h"
#include <cstdlib>

namespace mae {

namespace {

// ---------------------------------------------------------------------------------------------------
// the band walk's parts
// ---------------------------------------------------------------------------------------------------
// 0 = the band walk serves this geometry with n tokens per image and px_bytes per pixel; 1 = the patch shape does not fit (rows are
// moved four pixels at a time; the token list keeps the patch column in 8 bits, 0xff = class token); 2 = the band (<= 96 KiB) or the
// token list (<= 8192 entries) does not fit the LDS
int band_walk_misfit(int C, int img, int p, int n, int px_bytes) {
  if (!(p > 0 && img % p == 0 && p % 4 == 0 && img / p <= 64)) return 1;
  return (int64_t)C * p * img * px_bytes <= 96 * 1024 && n <= 8192 ? 0 : 2;
}

// The tokens of one band are listed in LDS behind the band image: n_tok slots, so that even an index list that names one
// band over and over (legal for a caller-made idx_keep) is served completely.

// band (b, ph) -> LDS image [C][p][W] pixels (W % 4 == 0), one word of four pixels per thread and pass: 4 bytes of uint8 ...
__device__ __forceinline__ void load_band(const uint8_t* __restrict__ images, int64_t b, int ph, int C, int img, int p, uint8_t* band) {
  const int wpr = img >> 2, words = C * p * wpr;
  for (int w = threadIdx.x; w < words; w += 256) {
    const int row = w / wpr, col = w - row * wpr;
    const int c = row / p, py = row - c * p;
    const unsigned* src = reinterpret_cast<const unsigned*>(images + ((b * C + c) * (int64_t)img + (ph * p + py)) * img);
    reinterpret_cast<unsigned*>(band)[w] = src[col];
  }
}
// ... 16 bytes of float.  The same walk, kept as its own loop: with the LDS address written as word w, as above, hipcc compiled a float
// loss that ran 1.6 % longer at batch 2000 (0.1541 against 0.1517 ms); this form gives the code that was measured before
__device__ __forceinline__ void load_band(const float* __restrict__ images, int64_t b, int ph, int C, int img, int p, float* band) {
  const int wpr = img >> 2;
  for (int w = threadIdx.x; w < C * p * wpr; w += 256) {
    const int row = w / wpr, col = w - row * wpr;
    const int c = row / p, py = row - c * p;
    store4(band + row * img + col * 4, load4(images + ((b * C + c) * (int64_t)img + (ph * p + py)) * img + col * 4));
  }
}

// tokens of image b that lie in band ph -> list (j index, patch column); class token (t == 0) belongs to band 0 when with_cls
template <class I>
__device__ __forceinline__ void band_tokens(const I* __restrict__ tok, int64_t b, int n_tok, int g, int ph, bool with_cls, int* list, int* cnt) {
  for (int j = threadIdx.x; j < n_tok; j += 256) {
    const int t = (int)tok[b * n_tok + j];
    bool mine;
    int pw;
    if (t <= 0 && with_cls) { mine = ph == 0; pw = -1; }  // class token: a zero row
    else {  // idx - 1 clamped into the patch grid (the reference's clamp(idx_mask - 1, min=0), src/models/mae.py:91)
      const int n = t <= 0 ? 0 : (t - 1 < g * g ? t - 1 : g * g - 1); mine = n / g == ph; pw = n - (n / g) * g;
    }
    if (mine) {
      const int slot = atomicAdd(cnt, 1);
      list[slot] = (j << 8) | (pw & 0xff);
    }
  }
}

// the list in ascending order (entries are distinct): a kernel that SUMS over the band's tokens then adds them in an order that does
// not depend on which thread won which slot -- the loss comes out bit-identical from run to run
__device__ __forceinline__ void sort_band_list(const int* list, int n, int* sorted) {
  for (int i = threadIdx.x; i < n; i += 256) {
    const int v = list[i];
    int rank = 0;
    for (int o = 0; o < n; ++o) rank += list[o] < v;
    sorted[rank] = v;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// visible-patch gather: out[(b, j)][c*p*p + py*p + px] = normalised pixel of patch tok[b][j]-1, zero row for the class token
// ---------------------------------------------------------------------------------------------------
template <class T, int VEC>
__global__ void __launch_bounds__(256) gather_patches_kernel(const float* __restrict__ images,
                                                             const int32_t* __restrict__ tok, int64_t rows, int k,
                                                             int C, int img, int p, T* __restrict__ out) {
  const int g = img / p;
  const int pv = p / VEC;                 // vector units per patch row
  const int units_per_row = C * p * pv;   // per token row
  const int64_t total = rows * units_per_row;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t r = u / units_per_row;
    int rem = (int)(u - r * units_per_row);
    const int c = rem / (p * pv);
    rem -= c * p * pv;
    const int py = rem / pv;
    const int px = (rem - py * pv) * VEC;
    const int t = tok[r];
    const int64_t b = r / k;
    T* dst = out + r * (int64_t)(C * p * p) + (c * p + py) * p + px;
    if (t <= 0) {
#pragma unroll
      for (int i = 0; i < VEC; ++i) dst[i] = from_f<T>(0.f);
    } else {
      const int n = t - 1, ph = n / g, pw = n - ph * g;
      const float* src = images + ((b * C + c) * (int64_t)img + (ph * p + py)) * img + pw * p + px;
      if (VEC == 4) {
        store4(dst, load4(src));
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) dst[i] = from_f<T>(src[i]);
      }
    }
  }
}

template <class T>
__global__ void __launch_bounds__(256) gather_patches_u8_kernel(const uint8_t* __restrict__ images, const int32_t* __restrict__ tok, int B,
                                                                int k, int C, int img, int p, T* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds32[];
  uint8_t* band = reinterpret_cast<uint8_t*>(lds32);
  int* list = reinterpret_cast<int*>(band + C * p * img);
  __shared__ int cnt;
  const int g = img / p, P = C * p * p, p4 = p >> 2, units = C * p * p4;
  for (int64_t bb = blockIdx.x; bb < (int64_t)B * g; bb += gridDim.x) {
    const int64_t b = bb / g;
    const int ph = (int)(bb - b * g);
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    load_band(images, b, ph, C, img, p, band);
    band_tokens(tok, b, k, g, ph, true, list, &cnt);
    __syncthreads();
    const int n = cnt;
    for (int it = threadIdx.x; it < n * units; it += 256) {
      const int li = it / units, u = it - li * units;
      const int j = list[li] >> 8, pw = list[li] & 0xff;
      const int c = u / (p * p4), rem = u - c * (p * p4);
      const int py = rem / p4, px = (rem - py * p4) << 2;
      T* dst = out + (b * k + j) * (int64_t)P + (c * p + py) * p + px;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (pw != 0xff) {
        const unsigned w = *reinterpret_cast<const unsigned*>(band + (c * p + py) * img + pw * p + px);
        v = f32x4{norm_u8(w & 0xff), norm_u8((w >> 8) & 0xff), norm_u8((w >> 16) & 0xff), norm_u8(w >> 24)};
      }
      store4(dst, v);
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------
// masked-pixel MSE against the image + dpred; element e of row r = (b, j) is (py, px, c) of patch clamp(mask[b][j]-1, 0, g*g-1).
// The per-pixel gather, the band walk and patchify_gather apply the same clamp: the variants agree on every id.
// ---------------------------------------------------------------------------------------------------
// One thread per (row, py, px): C strided pixels.
template <class T, bool HAS_GRAD>
__global__ void __launch_bounds__(256) mse_images_kernel(const float* __restrict__ pred,
                                                         const float* __restrict__ images,
                                                         const int32_t* __restrict__ mask32, int64_t rows, int m, int C,
                                                         int img, int p, float gscale, float* __restrict__ partial,
                                                         T* __restrict__ dpred) {
  __shared__ float red[4];
  const int g = img / p, pp = p * p;
  const int64_t total = rows * pp;
  float acc = 0.f;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t r = u / pp;
    const int q = (int)(u - r * pp);
    const int py = q / p, px = q - py * p;
    const int64_t b = r / m;
    int n = mask32[r] - 1;
    n = n < 0 ? 0 : (n >= g * g ? g * g - 1 : n);
    const int ph = n / g, pw = n - ph * g;
    const float* src = images + (b * C * (int64_t)img + (ph * p + py)) * img + pw * p + px;
    const int64_t o = r * (int64_t)(pp * C) + q * C;
    for (int c = 0; c < C; ++c) {
      const float d = pred[o + c] - src[(int64_t)c * img * img];
      acc += d * d;
      if (HAS_GRAD) dpred[o + c] = from_f<T>(d * gscale);
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// The band walk, PX = uint8_t or float: LDS = band, token list, its sorted copy.
template <class PX, class T, bool HAS_GRAD>
__global__ void __launch_bounds__(256) mse_images_band_kernel(const float* __restrict__ pred, const PX* __restrict__ images,
                                                              const int32_t* __restrict__ mask32, int B, int m, int C, int img, int p,
                                                              float gscale, float* __restrict__ partial, T* __restrict__ dpred) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds32[];
  PX* band = reinterpret_cast<PX*>(lds32);
  int* list = reinterpret_cast<int*>(band + C * p * img);
  int* sorted = list + m;   // the band's token list in ascending order
  __shared__ int cnt;
  __shared__ float red[4];
  const int g = img / p, P = C * p * p, p4 = p >> 2, units = p * p4;
  float acc = 0.f;
  for (int64_t bb = blockIdx.x; bb < (int64_t)B * g; bb += gridDim.x) {
    const int64_t b = bb / g;
    const int ph = (int)(bb - b * g);
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    load_band(images, b, ph, C, img, p, band);
    band_tokens(mask32, b, m, g, ph, false, list, &cnt);
    __syncthreads();
    const int n = cnt;
    sort_band_list(list, n, sorted);
    __syncthreads();
    for (int it = threadIdx.x; it < n * units; it += 256) {
      const int li = it / units, u = it - li * units;
      const int j = sorted[li] >> 8, pw = sorted[li] & 0xff;
      const int py = u / p4, px = (u - py * p4) << 2;
      const int64_t o = (b * m + j) * (int64_t)P + (py * p + px) * C;  // 4 pixels x C channels = 4C contiguous elements
      const PX* src = band + py * img + pw * p + px;
      for (int v = 0; v < C; ++v) {
        const f32x4 pr = load4(pred + o + 4 * v);
        f32x4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 4 * v + i, pxi = e / C, c = e - pxi * C;
          d[i] = pr[i] - px_value(src + c * p * img + pxi);
          acc += d[i] * d[i];
        }
        if (HAS_GRAD) store4(dpred + o + 4 * v, d * gscale);
      }
    }
    __syncthreads();
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <class PX>
static int mse_from_images_band(const float* pred, const PX* images, const int32_t* mask32, int B, int m, int C, int img, int p, float grad_scale,
                         float* loss, void* d_pred, int dpred_dt, float* scratch, hipStream_t s) {
  const int64_t n = (int64_t)B * m * p * p * C;
  const int grid = (int)std::min<int64_t>((int64_t)B * (img / p), RED_BLOCKS);
  const float gs = grad_scale * 2.0f / (float)n;
  const size_t lds = (size_t)C * p * img * sizeof(PX) + (size_t)m * 8;   // band + token list + its sorted copy: up to 96 + 64 KiB
  MAE_LAUNCH_LOSS(mse_images_band_kernel, (PX,), grid, lds, s, d_pred, dpred_dt, scratch, 1.0f / (float)n, loss, pred, images, mask32, B, m, C, img,
                  p, gs);
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// pixel targets: target[(b,j)][(py*p + px)*C + c] = images[b][c][ph*p+py][pw*p+px], patch = clamp(mask-1, 0, g*g-1): a class-token id
// (0) reads patch 0, like the reference's clamp (it never occurs in idx_mask)
// ---------------------------------------------------------------------------------------------------
// one thread per (row, py, px): reads C strided pixels, writes C contiguous floats
template <class I>
__global__ void __launch_bounds__(256) patchify_gather_kernel(const float* __restrict__ images,
                                                              const I* __restrict__ mask32, int64_t rows, int m,
                                                              int C, int img, int p, float* __restrict__ target) {
  const int g = img / p, pp = p * p;
  const int64_t total = rows * pp;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int64_t r = u / pp;
    const int q = (int)(u - r * pp);
    const int py = q / p, px = q - py * p;
    const int64_t b = r / m;
    int n = (int)mask32[r] - 1;
    n = n < 0 ? 0 : (n >= g * g ? g * g - 1 : n);
    const int ph = n / g, pw = n - ph * g;
    const float* src = images + (b * C * (int64_t)img + (ph * p + py)) * img + pw * p + px;
    float* dst = target + r * (int64_t)(pp * C) + q * C;
    for (int c = 0; c < C; ++c) dst[c] = src[(int64_t)c * img * img];
  }
}

template <class I>
__global__ void __launch_bounds__(256) patchify_gather_u8_kernel(const uint8_t* __restrict__ images, const I* __restrict__ mask, int B, int m,
                                                                 int C, int img, int p, float* __restrict__ target) {
  extern __shared__ __attribute__((aligned(16))) unsigned lds32[];
  uint8_t* band = reinterpret_cast<uint8_t*>(lds32);
  int* list = reinterpret_cast<int*>(band + C * p * img);
  __shared__ int cnt;
  const int g = img / p, P = C * p * p, p4 = p >> 2, units = p * p4;
  for (int64_t bb = blockIdx.x; bb < (int64_t)B * g; bb += gridDim.x) {
    const int64_t b = bb / g;
    const int ph = (int)(bb - b * g);
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    load_band(images, b, ph, C, img, p, band);
    band_tokens(mask, b, m, g, ph, false, list, &cnt);
    __syncthreads();
    const int n = cnt;
    for (int it = threadIdx.x; it < n * units; it += 256) {
      const int li = it / units, u = it - li * units;
      const int j = list[li] >> 8, pw = list[li] & 0xff;
      const int py = u / p4, px = (u - py * p4) << 2;
      const int64_t o = (b * m + j) * (int64_t)P + (py * p + px) * C;
      const uint8_t* src = band + py * img + pw * p + px;
      for (int v = 0; v < C; ++v) {
        f32x4 d;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int e = 4 * v + i, pxi = e / C, c = e - pxi * C;
          d[i] = norm_u8(src[c * p * img + pxi]);
        }
        store4(target + o + 4 * v, d);
      }
    }
    __syncthreads();
  }
}

template <class I>
static int patchify_gather_typed(const void* images, int img_dt, const I* mask, int B, int m, int C, int img, int p, float* target, hipStream_t s) {
  if (img_dt == MAE_U8) {
    MAE_REQUIRE(images && mask && target && B > 0 && m > 0, "patchify_gather(u8): bad arguments");
    MAE_REQUIRE(!band_walk_misfit(C, img, p, 0, 1), "uint8 images: unsupported geometry (image %d, patch %d)", img, p);
    MAE_REQUIRE(!band_walk_misfit(C, img, p, m, 1), "patchify_gather(u8): too many tokens per image");
    const int grid = (int)std::min<int64_t>((int64_t)B * (img / p), 256 * 16);
    const size_t lds = (size_t)C * p * img + (size_t)m * 4;
    MAE_TRY(allow_lds(patchify_gather_u8_kernel<I>, lds));
    hipLaunchKernelGGL((patchify_gather_u8_kernel<I>), dim3(grid), dim3(256), lds, s, (const uint8_t*)images, mask, B, m, C, img, p, target);
  } else {
    MAE_REQUIRE(images && mask && target && B > 0 && m > 0, "patchify_gather: bad arguments");
    MAE_REQUIRE(p > 0 && img % p == 0, "patchify: image_size %d not divisible by patch_size %d", img, p);
    const int64_t rows = (int64_t)B * m;
    const int grid = (int)std::min<int64_t>(cdiv(rows * p * p, 256), 256 * 16);
    hipLaunchKernelGGL((patchify_gather_kernel<I>), dim3(grid), dim3(256), 0, s, (const float*)images, mask, rows, m, C, img, p, target);
  }
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_gather_patches(const void* images, int img_dt, const int32_t* tok, int B, int k, int C, int img, int p, int dt, void* out,
                          hipStream_t s) {
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "mae_gather_patches: image_dtype must be MAE_F32 or MAE_U8 (got %d)", img_dt);
  if (img_dt == MAE_U8) {  // whole image rows through LDS: every pixel byte is fetched once
    MAE_REQUIRE(images && tok && out && B > 0 && k > 0, "gather_patches(u8): bad arguments");
    const int misfit = band_walk_misfit(C, img, p, k, 1);
    MAE_REQUIRE(misfit != 1, "uint8 images need patch_size %% 4 == 0 and at most 64 patches per side (got image %d, patch %d)", img, p);
    MAE_REQUIRE(misfit != 2, "uint8 images: one row of patches (%d bytes) does not fit the LDS band", C * p * img);
    const int grid = (int)std::min<int64_t>((int64_t)B * (img / p), 256 * 16);
    const size_t lds = (size_t)C * p * img + (size_t)k * 4;   // band + token list: up to 96 + 32 KiB
#define GP(T) MAE_TRY(allow_lds(gather_patches_u8_kernel<T>, lds)); hipLaunchKernelGGL((gather_patches_u8_kernel<T>), dim3(grid), dim3(256), lds, s, (const uint8_t*)images, tok, B, k, C, img, p, (T*)out)
    if (dt == MAE_BF16) { GP(bf16); } else { GP(float); }
#undef GP
  } else {
    MAE_REQUIRE(images && tok && out && B > 0 && k > 0, "gather_patches: bad arguments");
    MAE_REQUIRE(p > 0 && img % p == 0, "gather_patches: image_size %d not divisible by patch_size %d", img, p);
    const int64_t rows = (int64_t)B * k;
    const bool vec = (p % 4 == 0) && (img % 4 == 0);
    const int64_t units = rows * C * p * (vec ? p / 4 : p);
    const int grid = (int)std::min<int64_t>(cdiv(units, 256), 256 * 16);
#define GP(T, V) hipLaunchKernelGGL((gather_patches_kernel<T, V>), dim3(grid), dim3(256), 0, s, (const float*)images, tok, rows, k, C, img, p, (T*)out)
    if (dt == MAE_BF16) { if (vec) GP(bf16, 4); else GP(bf16, 1); }
    else                { if (vec) GP(float, 4); else GP(float, 1); }
#undef GP
  }
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_mse_from_images(const float* pred, const void* images, int img_dt, const int32_t* mask32, int B, int m, int C, int img, int p,
                           float grad_scale, float* loss, void* d_pred, int dpred_dt, float* scratch, int path, hipStream_t s) {
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "mae_mse_loss_from_images: image_dtype must be MAE_F32 or MAE_U8 (got %d)", img_dt);
  MAE_REQUIRE(path == 0 || (path == 1 && img_dt == MAE_F32), "mae_mse_loss_from_images: path must be 0, or 1 with MAE_F32 images (got %d)", path);
  MAE_REQUIRE(C > 0 && p > 0, "mae_mse_loss_from_images: bad arguments");
  if (img_dt == MAE_U8) {
    MAE_REQUIRE(pred && images && mask32 && loss && scratch && B > 0 && m > 0, "mse_from_images(u8): bad arguments");
    MAE_REQUIRE(!band_walk_misfit(C, img, p, m, 1), "uint8 images: unsupported geometry (image %d, patch %d)", img, p);
    return mse_from_images_band(pred, (const uint8_t*)images, mask32, B, m, C, img, p, grad_scale, loss, d_pred, dpred_dt, scratch, s);
  }
  MAE_REQUIRE(pred && images && mask32 && loss && scratch && B > 0 && m > 0 && p > 0 && img % p == 0, "mse_from_images: bad arguments");
  static const bool band = [] { const char* v = getenv("MAE_MSE_BAND"); return !v || v[0] != '0'; }();   // MAE_MSE_BAND=0: the per-pixel gather (A/B)
  // the band walk moves 16 bytes at a time: where a buffer or the row length is not aligned to that, the per-pixel gather serves
  const bool aligned = (((uintptr_t)pred | (uintptr_t)images | (uintptr_t)d_pred) & 15) == 0 && (C * p * p) % 4 == 0;
  if (path == 0 && band && aligned && !band_walk_misfit(C, img, p, m, 4))
    return mse_from_images_band(pred, (const float*)images, mask32, B, m, C, img, p, grad_scale, loss, d_pred, dpred_dt, scratch, s);
  const int64_t rows = (int64_t)B * m;
  const int64_t n = rows * p * p * C;
  const int grid = (int)std::min<int64_t>(cdiv(rows * p * p, 256), RED_BLOCKS);
  const float gs = grad_scale * 2.0f / (float)n;
  MAE_LAUNCH_LOSS(mse_images_kernel, (), grid, 0, s, d_pred, dpred_dt, scratch, 1.0f / (float)n, loss, pred, (const float*)images, mask32, rows, m, C,
                  img, p, gs);
  return 0;
}

int launch_patchify_gather(const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p, float* target,
                           hipStream_t s) {
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "mae_patchify_gather: image_dtype must be MAE_F32 or MAE_U8 (got %d)", img_dt);
  return idx64 ? patchify_gather_typed(images, img_dt, static_cast<const int64_t*>(idx), B, m, C, img, p, target, s)
               : patchify_gather_typed(images, img_dt, static_cast<const int32_t*>(idx), B, m, C, img, p, target, s);
}

// ---------------------------------------------------------------------------------------------------
// The augmentation step in front of the path (src/data.py:15-20: RandomResizedCrop(size, scale=(0.8, 1.0)) +
// RandomHorizontalFlip on the PIL uint8 image, before ToTensor): per image a crop box (top, left, h, w) and a flip flag are
// drawn on the host side (ssrl_vit_mae_jepa_amd/data.py: random_resized_crop_params) and this kernel resamples the box to
// the full size x size frame, bilinear, pixel centres aligned as F.grid_sample(align_corners=False, padding_mode="border")
// does, rounds to uint8 like the PIL resize and mirrors columns when flip is set.  uint8 in, uint8 out: the batch stays
// 1 B per pixel all the way into the engine's pixel readers.  One thread per output pixel, all channels.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) augment_crop_flip_u8_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ params,
                                                                   int B, int C, int S, uint8_t* __restrict__ out) {
  const int64_t total = (int64_t)B * S * S;
  const float inv2s = 0.5f / (float)S;
  for (int64_t u = blockIdx.x * 256ll + threadIdx.x; u < total; u += (int64_t)gridDim.x * 256) {
    const int b = (int)(u / (S * S));
    const int r = (int)(u - (int64_t)b * S * S);
    const int oy = r / S, ox = r - oy * S;
    const int top = params[5 * b + 0], left = params[5 * b + 1], h = params[5 * b + 2], w = params[5 * b + 3], flip = params[5 * b + 4];
    // source coordinate of the output pixel centre: left + w * (2 ox' + 1) / (2 S) - 0.5, ox' mirrored under a flip
    const int oxm = flip ? S - 1 - ox : ox;
    float fx = (float)left + (float)w * (float)(2 * oxm + 1) * inv2s - 0.5f;
    float fy = (float)top + (float)h * (float)(2 * oy + 1) * inv2s - 0.5f;
    fx = fminf(fmaxf(fx, 0.f), (float)(S - 1));   // border padding: coordinates are clipped before interpolation
    fy = fminf(fmaxf(fy, 0.f), (float)(S - 1));
    const int x0 = (int)floorf(fx), y0 = (int)floorf(fy);
    const int x1 = x0 + 1 < S ? x0 + 1 : S - 1, y1 = y0 + 1 < S ? y0 + 1 : S - 1;
    const float ax = fx - (float)x0, ay = fy - (float)y0;
    const float w00 = (1.f - ax) * (1.f - ay), w01 = ax * (1.f - ay), w10 = (1.f - ax) * ay, w11 = ax * ay;
    const uint8_t* src = in + (int64_t)b * C * S * S;
    uint8_t* dst = out + (int64_t)b * C * S * S + oy * S + ox;
    for (int c = 0; c < C; ++c) {
      const uint8_t* pc = src + (int64_t)c * S * S;
      const float v = w00 * (float)pc[y0 * S + x0] + w01 * (float)pc[y0 * S + x1] + w10 * (float)pc[y1 * S + x0] + w11 * (float)pc[y1 * S + x1];
      dst[(int64_t)c * S * S] = (uint8_t)(int)fminf(fmaxf(rintf(v), 0.f), 255.f);
    }
  }
}

int launch_augment_crop_flip_u8(const uint8_t* in, const int32_t* params, int B, int C, int S, uint8_t* out, hipStream_t s) {
  MAE_REQUIRE(in && params && out && B > 0 && C > 0 && S > 0, "augment_crop_flip_u8: bad arguments");
  MAE_REQUIRE(in != out, "augment_crop_flip_u8: in-place resampling is not supported");
  const int grid = (int)std::min<int64_t>(cdiv((int64_t)B * S * S, 256), 256 * 32);
  hipLaunchKernelGGL(augment_crop_flip_u8_kernel, dim3(grid), dim3(256), 0, s, in, params, B, C, S, out);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_gather_patches(const void* images, int32_t image_dtype, const int32_t* tok32, int32_t batch, int32_t num_keep, int32_t in_chans,
                                  int32_t image_size, int32_t patch_size, int32_t out_dtype, void* out, void* stream) {
  return mae::launch_gather_patches(images, image_dtype, tok32, batch, num_keep, in_chans, image_size, patch_size, out_dtype, out,
                                    (hipStream_t)stream);
}

extern "C" int mae_patchify_gather(const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch, int32_t in_chans,
                                   int32_t image_size, int32_t patch_size, int32_t num_mask, float* target, void* stream) {
  return mae::launch_patchify_gather(images, image_dtype, idx_mask, 1, batch, num_mask, in_chans, image_size, patch_size, target,
                                     (hipStream_t)stream);
}

extern "C" int mae_mse_loss_from_images(const float* pred, const void* images, int32_t image_dtype, const int32_t* mask32, int32_t batch,
                                        int32_t num_mask, int32_t in_chans, int32_t image_size, int32_t patch_size, float grad_scale, float* loss,
                                        void* d_pred, int32_t d_pred_dtype, float* scratch, int32_t path, void* stream) {
  return mae::launch_mse_from_images(pred, images, image_dtype, mask32, batch, num_mask, in_chans, image_size, patch_size, grad_scale, loss, d_pred,
                                     d_pred_dtype, scratch, path, (hipStream_t)stream);
}

extern "C" int mae_augment_crop_flip_u8(const uint8_t* images, const int32_t* params, int32_t batch, int32_t in_chans, int32_t image_size,
                                        uint8_t* out, void* stream) {
  return mae::launch_augment_crop_flip_u8(images, params, batch, in_chans, image_size, out, (hipStream_t)stream);
}
