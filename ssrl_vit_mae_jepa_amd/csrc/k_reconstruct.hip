// MAE reconstruction compose: the inverse of patchify_gather, fused with the whole-image error statistics.
// Reference behaviour (scripts/evaluation/visualize_reconstruction.py:127-334, MAEReconstructor):
//   _create_masked_images      == patchify(images) -> set_at_index(idx_mask - 1, 0.5) -> unpatchify      (:170-190)
//   _reconstruct_full_images   == patchify(images) -> set_at_index(idx_mask - 1, x_pred) -> unpatchify   (:198-234)
//   _tensor_to_image           == clamp(v * 0.5 + 0.5, 0, 1)                                             (:311-322)
//   nn.MSELoss / nn.L1Loss(original, reconstructed) over whole images                                    (:324-334)
// The reference walks patch space (six full-size temporaries); here the walk is over OUTPUT pixels: an inverse map says for
// every patch whether (and by which pred row) it is replaced, and every output byte is written exactly once, coalesced NCHW.
// Data movement only: images read once, pred read once, each requested output written once (timing not measured: DESIGN section 12).
#include "kernels.h"

namespace mae {

namespace {

constexpr int RC_UPT = 2;               // units per thread and work item
constexpr int RC_CHUNK = 256 * RC_UPT;  // units per work item: fixed, so the summation order of an image depends on its shape alone

// inv[b][n] = -1, then inv[b][idx_mask[b][j] - 1] = j for entries in [1, N].  One workgroup per image.  Entries <= 0 (the class
// token) and > N are compared as int64 and never become an index (the reference's __remove_cls_token, :192-196).
__global__ void __launch_bounds__(256) build_patch_inverse_kernel(const int64_t* __restrict__ mask, int m, int N, int32_t* __restrict__ inv) {
  const int b = blockIdx.x;
  int32_t* row = inv + (int64_t)b * N;
  for (int n = threadIdx.x; n < N; n += 256) row[n] = -1;
  __syncthreads();
  for (int j = threadIdx.x; j < m; j += 256) {
    const int64_t t = mask[(int64_t)b * m + j];
    if (t >= 1 && t <= (int64_t)N) row[t - 1] = j;
  }
}

// V normalised pixels of one row
template <int V> __device__ __forceinline__ void load_px(const float* __restrict__ p, float (&o)[V]) {
  if constexpr (V == 4) { const f32x4 v = load4(p); o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = v[3]; }
  else o[0] = p[0];
}
template <int V> __device__ __forceinline__ void load_px(const uint8_t* __restrict__ p, float (&o)[V]) {
  if constexpr (V == 4) {
    const unsigned w = *reinterpret_cast<const unsigned*>(p);
    o[0] = norm_u8(w & 0xff); o[1] = norm_u8((w >> 8) & 0xff); o[2] = norm_u8((w >> 16) & 0xff); o[3] = norm_u8(w >> 24);
  } else o[0] = norm_u8(p[0]);
}

// display pixel of a normalised value: round_half_even(clamp(v * 0.5 + 0.5, 0, 1) * 255).  v * 0.5 is exact, so the sum rounds once
// with or without FMA contraction; v_rndne is round-half-even.
__device__ __forceinline__ unsigned display_u8(float v) { return (unsigned)rintf(fminf(fmaxf(v * 0.5f + 0.5f, 0.f), 1.f) * 255.0f); }

template <int V> __device__ __forceinline__ void store_px(float* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4) store4(p, f32x4{v[0], v[1], v[2], v[3]});
  else p[0] = v[0];
}
template <int V> __device__ __forceinline__ void store_px(uint8_t* __restrict__ p, const float (&v)[V]) {
  if constexpr (V == 4)
    *reinterpret_cast<unsigned*>(p) = display_u8(v[0]) | (display_u8(v[1]) << 8) | (display_u8(v[2]) << 16) | (display_u8(v[3]) << 24);
  else p[0] = (uint8_t)display_u8(v[0]);
}

// Work item = (image, chunk of RC_CHUNK units); unit = V contiguous pixels of one image row, in every channel: the thread
// walks the C planes, so its pred reads are one contiguous run of V * C floats and each plane access is coalesced across the
// wave.  partial[item] = {sum d^2, sum |d|} over the item's replaced pixels, reduced in a fixed order.
template <class IN, class OUT, int V>
__global__ void __launch_bounds__(256) reconstruct_compose_kernel(const IN* __restrict__ images, const float* __restrict__ pred,
                                                                  const int32_t* __restrict__ inv, int items, int chunks, int C, int S, int p,
                                                                  int m, float fill, OUT* __restrict__ recon, OUT* __restrict__ masked,
                                                                  float* __restrict__ partial) {
  __shared__ float red[8];
  // 32-bit index math only (see decoder_assemble_kernel): items = B * chunks and B * N are < 2^31 (checked by the launcher)
  const int g = S / p, N = g * g, sv = S / V, units = S * sv;
  const int64_t plane = (int64_t)S * S;
  for (int it = blockIdx.x; it < items; it += gridDim.x) {
    const int b = (int)((uint32_t)it / (uint32_t)chunks);
    const int ch = it - b * chunks;
    float sq = 0.f, ab = 0.f;
#pragma unroll
    for (int r = 0; r < RC_UPT; ++r) {
      const int u = ch * RC_CHUNK + r * 256 + threadIdx.x;
      if (u < units) {
        const int y = (int)((uint32_t)u / (uint32_t)sv), x = (u - y * sv) * V;
        const int ph = (int)((uint32_t)y / (uint32_t)p), py = y - ph * p;
        const int pw = (int)((uint32_t)x / (uint32_t)p), px = x - pw * p;
        const int j = inv[b * N + ph * g + pw];
        const int64_t pix = (int64_t)b * C * plane + y * S + x;
        const float* __restrict__ q = pred + (((int64_t)b * m + (j < 0 ? 0 : j)) * (p * p) + py * p + px) * C;
        for (int c = 0; c < C; ++c) {
          float o[V], rv[V], mv[V];
          load_px<V>(images + pix + c * plane, o);
#pragma unroll
          for (int i = 0; i < V; ++i) {
            if (j >= 0) {
              const float pv = q[i * C + c];
              const float d = pv - o[i];
              sq += d * d;
              ab += fabsf(d);
              rv[i] = pv;
              mv[i] = fill;
            } else {
              rv[i] = o[i];
              mv[i] = o[i];
            }
          }
          if (recon) store_px<V>(recon + pix + c * plane, rv);
          if (masked) store_px<V>(masked + pix + c * plane, mv);
        }
      }
    }
    if (partial) {  // uniform over the grid
      sq = block_sum_256(sq, red);
      ab = block_sum_256(ab, red + 4);
      if (threadIdx.x == 0) { partial[2 * (int64_t)it] = sq; partial[2 * (int64_t)it + 1] = ab; }
    }
  }
}

// second stage: one thread per image adds its chunks in chunk order
__global__ void __launch_bounds__(256) reconstruct_stats_kernel(const float* __restrict__ partial, int B, int chunks, float* __restrict__ stats) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b >= B) return;
  float sq = 0.f, ab = 0.f;
  for (int i = 0; i < chunks; ++i) {
    sq += partial[2 * ((int64_t)b * chunks + i)];
    ab += partial[2 * ((int64_t)b * chunks + i) + 1];
  }
  stats[2 * b] = sq;
  stats[2 * b + 1] = ab;
}

inline bool rc_vec(int S, int p) { return p % 4 == 0 && S % 4 == 0; }
inline int rc_chunks(int S, int p) { return (int)cdiv((int64_t)S * (S / (rc_vec(S, p) ? 4 : 1)), RC_CHUNK); }
inline int64_t rc_inv_bytes(int B, int S, int p) { return round_up((int64_t)B * (S / p) * (S / p) * 4, 256); }

}  // namespace

int64_t reconstruct_scratch_bytes(int B, int C, int S, int p) {
  if (B <= 0 || C <= 0 || S <= 0 || p <= 0 || S % p != 0 || S > 16384) return -1;
  if ((int64_t)B * (S / p) * (S / p) >= (1ll << 31) || (int64_t)B * rc_chunks(S, p) >= (1ll << 31)) return -1;
  return rc_inv_bytes(B, S, p) + round_up((int64_t)B * rc_chunks(S, p) * 2 * 4, 256);
}

int check_reconstruct_compose(const void* images, int img_dt, const float* pred, const int64_t* idx_mask, int B, int C, int S, int p, int m,
                              int out_dt, const void* recon, const void* masked, const float* stats, const void* scratch,
                              int64_t scratch_bytes) {
  MAE_REQUIRE(img_dt == MAE_F32 || img_dt == MAE_U8, "reconstruct_compose: image_dtype must be MAE_F32 or MAE_U8 (got %d)", img_dt);
  MAE_REQUIRE(out_dt == MAE_F32 || out_dt == MAE_U8, "reconstruct_compose: out_dtype must be MAE_F32 or MAE_U8 (got %d)", out_dt);
  MAE_REQUIRE(B > 0 && C > 0 && S > 0 && p > 0 && S <= 16384, "reconstruct_compose: bad batch %d / in_chans %d / image_size %d / patch_size %d", B, C, S, p);
  MAE_REQUIRE(S % p == 0, "reconstruct_compose: image_size %d not divisible by patch_size %d", S, p);
  MAE_REQUIRE(m >= 1, "reconstruct_compose: num_mask must be >= 1 (got %d)", m);
  MAE_REQUIRE((int64_t)B * (S / p) * (S / p) < (1ll << 31) && (int64_t)B * rc_chunks(S, p) < (1ll << 31),
              "reconstruct_compose: batch * num_patches must be < 2^31");
  MAE_REQUIRE(images && pred && idx_mask && scratch, "reconstruct_compose: null images/pred/idx_mask/scratch");
  MAE_REQUIRE(recon || masked || stats, "reconstruct_compose: no output requested");
  // no output may overlap an input or the other output, in whole or in part
  const int64_t px = (int64_t)B * C * S * S;
  const int64_t in_bytes = px * (img_dt == MAE_U8 ? 1 : 4), out_bytes = px * (out_dt == MAE_U8 ? 1 : 4), pred_bytes = (int64_t)B * m * p * p * C * 4;
  auto overlap = [](const void* a, int64_t na, const void* b, int64_t nb) {
    return a && b && (uintptr_t)a < (uintptr_t)b + (uintptr_t)nb && (uintptr_t)b < (uintptr_t)a + (uintptr_t)na;
  };
  MAE_REQUIRE(!overlap(recon, out_bytes, images, in_bytes) && !overlap(masked, out_bytes, images, in_bytes),
              "reconstruct_compose: an output may not overlap images (out != images)");
  MAE_REQUIRE(!overlap(recon, out_bytes, pred, pred_bytes) && !overlap(masked, out_bytes, pred, pred_bytes),
              "reconstruct_compose: an output may not overlap pred");
  MAE_REQUIRE(!overlap(recon, out_bytes, masked, out_bytes), "reconstruct_compose: recon and masked must be different buffers");
  MAE_REQUIRE(scratch_bytes >= reconstruct_scratch_bytes(B, C, S, p), "reconstruct_compose: scratch too small (%lld < %lld bytes)",
              (long long)scratch_bytes, (long long)reconstruct_scratch_bytes(B, C, S, p));
  // vector path: 16-byte image / output accesses (uint8: 4-byte); pred is read float by float
  const uintptr_t align = rc_vec(S, p) ? 15 : 3;
  MAE_REQUIRE(((uintptr_t)scratch & 255) == 0 && ((uintptr_t)pred & 3) == 0 && ((uintptr_t)images & (img_dt == MAE_U8 ? align >> 2 : align)) == 0 &&
                  ((uintptr_t)recon & (out_dt == MAE_U8 ? align >> 2 : align)) == 0 && ((uintptr_t)masked & (out_dt == MAE_U8 ? align >> 2 : align)) == 0,
              "reconstruct_compose: scratch must be 256-byte aligned, fp32 images / outputs 16-byte (4-byte when patch_size or image_size is "
              "no multiple of 4), uint8 ones 4-byte (1-byte), pred 4-byte");
  return 0;
}

int launch_reconstruct_compose(const void* images, int img_dt, const float* pred, const int64_t* idx_mask, int B, int C, int S, int p, int m,
                               float fill, int out_dt, void* recon, void* masked, float* stats, void* scratch, int64_t scratch_bytes,
                               hipStream_t s) {
  MAE_TRY(check_reconstruct_compose(images, img_dt, pred, idx_mask, B, C, S, p, m, out_dt, recon, masked, stats, scratch, scratch_bytes));
  const int N = (S / p) * (S / p), chunks = rc_chunks(S, p), items = B * chunks;
  int32_t* inv = reinterpret_cast<int32_t*>(scratch);
  float* partial = stats ? reinterpret_cast<float*>(reinterpret_cast<char*>(scratch) + rc_inv_bytes(B, S, p)) : nullptr;
  hipLaunchKernelGGL(build_patch_inverse_kernel, dim3(B), dim3(256), 0, s, idx_mask, m, N, inv);
  MAE_LAUNCH_CHECK();
  const int grid = std::min(items, 256 * 64);
#define RC(IN, OUT, V)                                                                                                              \
  hipLaunchKernelGGL((reconstruct_compose_kernel<IN, OUT, V>), dim3(grid), dim3(256), 0, s, (const IN*)images, pred, inv, items, chunks, C, \
                     S, p, m, fill, (OUT*)recon, (OUT*)masked, partial)
  const bool vec = rc_vec(S, p), in8 = img_dt == MAE_U8, out8 = out_dt == MAE_U8;
  if (vec) {
    if (in8) { if (out8) RC(uint8_t, uint8_t, 4); else RC(uint8_t, float, 4); }
    else     { if (out8) RC(float, uint8_t, 4);   else RC(float, float, 4); }
  } else {
    if (in8) { if (out8) RC(uint8_t, uint8_t, 1); else RC(uint8_t, float, 1); }
    else     { if (out8) RC(float, uint8_t, 1);   else RC(float, float, 1); }
  }
#undef RC
  MAE_LAUNCH_CHECK();
  if (stats) {
    hipLaunchKernelGGL(reconstruct_stats_kernel, dim3((unsigned)cdiv(B, 256)), dim3(256), 0, s, partial, B, chunks, stats);
    MAE_LAUNCH_CHECK();
  }
  return 0;
}

}  // namespace mae

extern "C" int64_t mae_reconstruct_scratch_bytes(int32_t batch, int32_t in_chans, int32_t image_size, int32_t patch_size) {
  return mae::reconstruct_scratch_bytes(batch, in_chans, image_size, patch_size);
}

extern "C" int mae_reconstruct_compose(const void* images, int32_t image_dtype, const float* pred, const int64_t* idx_mask, int32_t batch,
                                       int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float fill,
                                       int32_t out_dtype, void* recon, void* masked, float* stats, void* scratch, int64_t scratch_bytes,
                                       void* stream) {
  return mae::launch_reconstruct_compose(images, image_dtype, pred, idx_mask, batch, in_chans, image_size, patch_size, num_mask, fill,
                                         out_dtype, recon, masked, stats, scratch, scratch_bytes, (hipStream_t)stream);
}
