// Downstream classifier: pooled linear head + cross-entropy (forward and backward) and the full-sequence embedding
// gradient, over [cls | patches] or the patch tokens alone (classifier_head_range_kernel, the HAS_CLS = false split).
// Reference: src/models/classifier.py:47-57 (pool + head), src/training/classifier.py:75-105 (F.cross_entropy, accuracy),
// src/training/classifier.py:134 (unfreeze_encoder: cls_token, pos_embed and the patch projection train too).
//
// bf16 engine rounding points (each one a GEMM operand of the head, fp32 accumulation everywhere):
//   (1) the pooled feature vector  -- with "mean" the rows are the engine's bf16 LayerNorm outputs, summed in fp32, then rounded;
//   (2) the head weight W          -- rounded as it is read (the head's fp32 buffer has no bf16 copy);
//   (3) d_logits                   -- rounded before dW, db and d_pooled are formed from it.
// The feature gradient leaves in the activation dtype (the input of the final LayerNorm backward), as every other dy does.
//
// Soft targets (SOFT = true: mixup / CutMix label pairs and label smoothing, the MAE / DeiT fine-tuning loss):
//   t[b][c] = eps / C + (1 - eps) * (lam[b] * [c == ya[b]] + (1 - lam[b]) * [c == yb[b]]),  sum_c t = 1, so
//   row_loss = lse - sum_c t[c] * logit[c]  and  d_logits = (softmax - t) * grad_scale / B, rounded at the same point (3).
// SOFT = false is the hard-label head as it always was: the launcher picks it whenever no soft option is active.
#include "kernels.h"

namespace mae {

template <class T> __device__ __forceinline__ float head_round(float x) { return x; }
template <> __device__ __forceinline__ float head_round<bf16>(float x) { return (float)(bf16)x; }

// The phases both head kernels share once the pooled vector sits in sp[0 .. D): logits, row loss / correct flag, d_logits and
// the pooled copy.  Wave w owns classes w, w+4, ...; returns false when the caller has nothing left to do (no backward asked).
template <class T, bool SOFT>
__device__ __forceinline__ bool head_after_pool(const float* sp, float* sl, float* sdl, float* sstat, int* sy, int b, int D,
                                                const float* __restrict__ W, const float* __restrict__ bias, int C,
                                                const int64_t* __restrict__ labels, const HeadSoft soft, float grad_scale, int B,
                                                float* __restrict__ logits_out, float* __restrict__ row_loss,
                                                int32_t* __restrict__ row_correct, float* __restrict__ pooled_out,
                                                float* __restrict__ dlogits_out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D4 = D / 4;
  // logits = pooled @ W.T + b
  for (int c = wave; c < C; c += 4) {
    float acc = 0.f;
    for (int q = lane; q < D4; q += 64) {
      const f32x4 w = load4(W + (int64_t)c * D + 4 * q);
      for (int i = 0; i < 4; ++i) acc += head_round<T>(w[i]) * sp[4 * q + i];  // rounding point (2)
    }
    acc = wave_sum(acc);
    if (lane == 0) sl[c] = acc + bias[c];
  }
  __syncthreads();
  if (t == 0) {
    // max-subtracted log-sum-exp; argmax keeps the first index among equal maxima (torch.argmax)
    float mx = sl[0];
    int am = 0;
    for (int c = 1; c < C; ++c)
      if (sl[c] > mx) { mx = sl[c]; am = c; }
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(sl[c] - mx);
    const float lse = mx + logf(se);
    const int64_t y = labels ? labels[b] : -1;
    sstat[0] = lse;
    if constexpr (SOFT) {
      const int64_t yb = soft.labels_b ? soft.labels_b[b] : y;
      const float lam = soft.lam ? soft.lam[b] : 1.f;
      const bool ya_ok = y >= 0 && y < C;
      const bool valid = ya_ok && yb >= 0 && yb < C;  // either label out of range: never an index, the row's loss is NaN
      sy[0] = valid ? (int)y : -1;
      sy[1] = valid ? (int)yb : -1;
      sstat[1] = lam;
      float dot = __builtin_nanf("");
      if (valid) {  // sum_c t[c] * logit[c]: the classes in ascending order, then the two label terms
        float all = 0.f;
        for (int c = 0; c < C; ++c) all += sl[c];
        dot = soft.eps / (float)C * all + (1.f - soft.eps) * (lam * sl[y] + (1.f - lam) * sl[yb]);
      }
      row_loss[b] = lse - dot;
      row_correct[b] = (ya_ok && am == (int)y) ? 1 : 0;
    } else {
      const bool valid = y >= 0 && y < C;   // an out-of-range label is never used as an index: its row's loss is NaN
      sy[0] = valid ? (int)y : -1;
      row_loss[b] = valid ? lse - sl[y] : __builtin_nanf("");
      row_correct[b] = (valid && am == (int)y) ? 1 : 0;
    }
  }
  __syncthreads();
  if (logits_out)
    for (int c = t; c < C; c += 256) logits_out[(int64_t)b * C + c] = sl[c];
  if (!dlogits_out) return false;
  // d_logits = (softmax - onehot(y)) * grad_scale / B
  const float lse = sstat[0];
  const int y = sy[0];
  for (int c = t; c < C; c += 256) {
    float tgt = c == y ? 1.f : 0.f;
    if constexpr (SOFT) {
      const float lam = sstat[1];
      tgt = soft.eps / (float)C + (1.f - soft.eps) * (lam * tgt + (1.f - lam) * (c == sy[1] ? 1.f : 0.f));
    }
    float g = (expf(sl[c] - lse) - tgt) * grad_scale / (float)B;
    if (y < 0) g = __builtin_nanf("");
    g = head_round<T>(g);  // rounding point (3)
    sdl[c] = g;
    dlogits_out[(int64_t)b * C + c] = g;
  }
  if (t < D4) store4(pooled_out + (int64_t)b * D + 4 * t, f32x4{sp[4 * t], sp[4 * t + 1], sp[4 * t + 2], sp[4 * t + 3]});
  return true;
}

// columns [4t, 4t+4) of d_pooled = d_logits . W (W rounded as it is read)
template <class T>
__device__ __forceinline__ f32x4 head_dpooled(const float* sdl, const float* __restrict__ W, int C, int D, int t) {
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    const f32x4 w = load4(W + (int64_t)c * D + 4 * t);
    const f32x4 wr = {head_round<T>(w[0]), head_round<T>(w[1]), head_round<T>(w[2]), head_round<T>(w[3])};
    acc += sdl[c] * wr;
  }
  return acc;
}

// One block per image.  Thread t owns feature columns [4t, 4t+4) (t < D/4); wave w owns classes w, w+4, ...
template <class T, bool SOFT>
__global__ void __launch_bounds__(256) classifier_head_kernel(const T* __restrict__ feats, int L, int D, int pool,
                                                              const float* __restrict__ W, const float* __restrict__ bias, int C,
                                                              const int64_t* __restrict__ labels, const HeadSoft soft, float grad_scale, int B,
                                                              float* __restrict__ logits_out, float* __restrict__ row_loss,
                                                              int32_t* __restrict__ row_correct, float* __restrict__ pooled_out,
                                                              float* __restrict__ dlogits_out, T* __restrict__ dfeat_out,
                                                              const float* __restrict__ mean_all, const float* __restrict__ rstd_all,
                                                              float* __restrict__ mean_c, float* __restrict__ rstd_c,
                                                              int32_t* __restrict__ cls_rows) {
  __shared__ __attribute__((aligned(16))) float sp[1024];
  __shared__ float sl[HEAD_MAX_CLASSES], sdl[HEAD_MAX_CLASSES], sstat[2];
  __shared__ int sy[2];
  const int b = blockIdx.x, t = threadIdx.x;
  const int D4 = D / 4;
  const int64_t row0 = (int64_t)b * L;
  // pooled features: feats[:, 0] or feats.mean(dim=1) over all L rows (class token included)
  if (t < D4) {
    f32x4 v;
    if (pool == MAE_POOL_CLS) {
      v = load4(feats + row0 * D + 4 * t);
    } else {
      v = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int j = 0; j < L; ++j) v += load4(feats + (row0 + j) * D + 4 * t);
      v = v / (float)L;
    }
    for (int i = 0; i < 4; ++i) sp[4 * t + i] = head_round<T>(v[i]);  // rounding point (1)
  }
  if (t == 0 && cls_rows) {  // compact statistics of the class-token rows for the row-mapped final LayerNorm backward
    cls_rows[b] = (int32_t)row0;
    mean_c[b] = mean_all[row0];
    rstd_c[b] = rstd_all[row0];
  }
  __syncthreads();
  if (!head_after_pool<T, SOFT>(sp, sl, sdl, sstat, sy, b, D, W, bias, C, labels, soft, grad_scale, B, logits_out, row_loss, row_correct, pooled_out,
                          dlogits_out))
    return;
  if (!dfeat_out) return;
  __syncthreads();
  // d_pooled = d_logits . W  ->  cls: row 0 of the image only (compact, row-mapped by the caller); mean: d_pooled / L on every row
  if (t < D4) {
    f32x4 acc = head_dpooled<T>(sdl, W, C, D, t);
    if (pool == MAE_POOL_CLS) {
      store4(dfeat_out + (int64_t)b * D + 4 * t, acc);
    } else {
      acc = acc / (float)L;
      for (int j = 0; j < L; ++j) store4(dfeat_out + (row0 + j) * D + 4 * t, acc);
    }
  }
}

// The same head over the mean of rows [lo, hi) of each image's `seq` rows: a patch-only sequence (lo = 0) or the patch rows
// behind a class token (lo = 1).  All four waves load rows: wave w sums rows lo + w, lo + w + 4, ... (lane l owns the 4-column
// groups l, l + 64, ...), and the four partial sums are added through LDS in wave order 0, 1, 2, 3, so the summation order is
// fixed by (lo, hi) alone.  The feature gradient is d_pooled / (hi - lo) on the pooled rows and exact zeros on the others.
template <class T, bool SOFT>
__global__ void __launch_bounds__(256) classifier_head_range_kernel(const T* __restrict__ feats, int seq, int D, int lo, int hi,
                                                                    const float* __restrict__ W, const float* __restrict__ bias, int C,
                                                                    const int64_t* __restrict__ labels, const HeadSoft soft, float grad_scale, int B,
                                                                    float* __restrict__ logits_out, float* __restrict__ row_loss,
                                                                    int32_t* __restrict__ row_correct, float* __restrict__ pooled_out,
                                                                    float* __restrict__ dlogits_out, T* __restrict__ dfeat_out) {
  __shared__ __attribute__((aligned(16))) float sp[1024];
  __shared__ __attribute__((aligned(16))) float part[3][1024];  // the partial sums of waves 1..3; then d_pooled in part[0]
  __shared__ float sl[HEAD_MAX_CLASSES], sdl[HEAD_MAX_CLASSES], sstat[2];
  __shared__ int sy[2];
  constexpr int Q = 4;  // 4-column groups per lane: D / 4 <= 256 = 64 * Q
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D4 = D / 4;
  const int64_t row0 = (int64_t)b * seq;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[Q] = {z, z, z, z};
#pragma unroll 2
  for (int j = lo + wave; j < hi; j += 4) {
    const T* row = feats + (row0 + j) * D;
#pragma unroll
    for (int i = 0; i < Q; ++i)
      if (lane + 64 * i < D4) acc[i] += load4(row + 4 * (lane + 64 * i));
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < Q; ++i)
      if (lane + 64 * i < D4) store4(&part[wave - 1][4 * (lane + 64 * i)], acc[i]);
  }
  __syncthreads();
  if (wave == 0) {
    const float n = (float)(hi - lo);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const int q = lane + 64 * i;
      if (q < D4) {
        f32x4 v = acc[i];
        for (int w = 0; w < 3; ++w) v += load4(&part[w][4 * q]);
        v = v / n;
        for (int k = 0; k < 4; ++k) sp[4 * q + k] = head_round<T>(v[k]);  // rounding point (1)
      }
    }
  }
  __syncthreads();
  if (!head_after_pool<T, SOFT>(sp, sl, sdl, sstat, sy, b, D, W, bias, C, labels, soft, grad_scale, B, logits_out, row_loss, row_correct, pooled_out,
                          dlogits_out))
    return;
  if (!dfeat_out) return;
  __syncthreads();
  if (t < D4) store4(&part[0][4 * t], head_dpooled<T>(sdl, W, C, D, t) / (float)(hi - lo));
  __syncthreads();
  for (int j = wave; j < seq; j += 4) {
    T* row = dfeat_out + (row0 + j) * D;
    const bool pooled = j >= lo && j < hi;
#pragma unroll
    for (int i = 0; i < Q; ++i) {
      const int q = lane + 64 * i;
      if (q < D4) store4(row + 4 * q, pooled ? load4(&part[0][4 * q]) : z);
    }
  }
}

// loss = mean of the row losses, correct = count of correct rows: one block, fixed summation order
__global__ void __launch_bounds__(256) classifier_reduce_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ row_correct,
                                                                int B, float* __restrict__ loss_out, int32_t* __restrict__ correct_out) {
  __shared__ float sl[256];
  __shared__ int sc[256];
  const int t = threadIdx.x;
  float l = 0.f;
  int n = 0;
  for (int b = t; b < B; b += 256) { l += row_loss[b]; n += row_correct[b]; }
  sl[t] = l; sc[t] = n;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { sl[t] += sl[t + w]; sc[t] += sc[t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    if (loss_out) loss_out[0] = sl[0] / (float)B;
    if (correct_out) correct_out[0] = sc[0];
  }
}

int check_pool(int with_cls, int pool, bool extended, const char* who) {
  if (!extended) {
    MAE_REQUIRE(pool == MAE_POOL_CLS || pool == MAE_POOL_MEAN, "%s: pool must be MAE_POOL_CLS or MAE_POOL_MEAN (got %d)", who, pool);
    return 0;
  }
  MAE_REQUIRE(with_cls == 0 || with_cls == 1, "%s: with_cls must be 0 or 1 (got %d)", who, with_cls);
  MAE_REQUIRE(pool == MAE_POOL_CLS || pool == MAE_POOL_MEAN || pool == MAE_POOL_MEAN_PATCHES,
              "%s: pool must be MAE_POOL_CLS, MAE_POOL_MEAN or MAE_POOL_MEAN_PATCHES (got %d)", who, pool);
  MAE_REQUIRE(pool != MAE_POOL_CLS || with_cls, "%s: MAE_POOL_CLS needs with_cls = 1 (a patch-only sequence has no class token)", who);
  return 0;
}

int launch_classifier_head(const HeadCall& h, hipStream_t s) {
  const bool range = h.range();  // the mean over the patch rows [lo, seq)
  const char* who = range ? "classifier_head_range" : "classifier_head";
  const int B = h.B, lo = h.with_cls ? 1 : 0;
  MAE_REQUIRE(h.feats && h.W && h.bias && h.row_loss && h.row_correct && B > 0 && h.seq > 0, "%s: bad arguments", who);
  MAE_TRY(check_pool(h.with_cls, h.pool, true, who));
  MAE_REQUIRE(!range || lo < h.seq, "%s: rows [%d, %d) outside the sequence of %d", who, lo, h.seq, h.seq);
  MAE_REQUIRE(h.D % 4 == 0 && h.D >= 4 && h.D <= 1024, "%s: D = %d must be a multiple of 4 in [4, 1024]", who, h.D);
  MAE_REQUIRE(h.C >= 2 && h.C <= HEAD_MAX_CLASSES, "%s: num_classes = %d outside [2, %d]", who, h.C, HEAD_MAX_CLASSES);
  MAE_REQUIRE(!h.dlogits_out || h.pooled_out, "%s: the backward needs the pooled-feature buffer", who);
  MAE_REQUIRE(!h.dfeat_out || h.dlogits_out, "%s: the feature gradient needs d_logits", who);
  MAE_REQUIRE(!h.cls_rows || (!range && h.mean_all && h.rstd_all && h.mean_c && h.rstd_c), "%s: class-row statistics need every buffer", who);
  const bool on = h.soft.active();
  MAE_REQUIRE(!on || (h.labels && h.soft.eps >= 0.f && h.soft.eps < 1.f), "%s: soft targets need labels and label_smoothing in [0, 1)", who);
  const HeadSoft hs = on ? h.soft : HeadSoft{nullptr, nullptr, 0.f};
#define HEAD(T, SOFT)                                                                                                                          \
  do {                                                                                                                                         \
    if (range)                                                                                                                                 \
      hipLaunchKernelGGL((classifier_head_range_kernel<T, SOFT>), dim3(B), dim3(256), 0, s, (const T*)h.feats, h.seq, h.D, lo, h.seq, h.W,     \
                         h.bias, h.C, h.labels, hs, h.grad_scale, B, h.logits_out, h.row_loss, h.row_correct, h.pooled_out, h.dlogits_out,     \
                         (T*)h.dfeat_out);                                                                                                     \
    else                                                                                                                                       \
      hipLaunchKernelGGL((classifier_head_kernel<T, SOFT>), dim3(B), dim3(256), 0, s, (const T*)h.feats, h.seq, h.D, h.pool, h.W, h.bias, h.C, \
                         h.labels, hs, h.grad_scale, B, h.logits_out, h.row_loss, h.row_correct, h.pooled_out, h.dlogits_out,                  \
                         (T*)h.dfeat_out, h.mean_all, h.rstd_all, h.mean_c, h.rstd_c, h.cls_rows);                                             \
  } while (0)
  if (on) { if (h.dt == MAE_BF16) HEAD(bf16, true); else HEAD(float, true); }
  else    { if (h.dt == MAE_BF16) HEAD(bf16, false); else HEAD(float, false); }
#undef HEAD
  MAE_LAUNCH_CHECK();
  if (h.loss_out || h.correct_out) {
    hipLaunchKernelGGL(classifier_reduce_kernel, dim3(1), dim3(256), 0, s, h.row_loss, h.row_correct, B, h.loss_out, h.correct_out);
    MAE_LAUNCH_CHECK();
  }
  return 0;
}

// Head weight gradient: column j < C*D is dW[j / D][j % D], column C*D + c is db[c]; grid.y = batch slices.
// partial[slice][j] = sum over the slice's rows in ascending order (launch_sum_partials then adds the slices in order).
__global__ void __launch_bounds__(256) classifier_head_wgrad_kernel(const float* __restrict__ dlogits, const float* __restrict__ pooled,
                                                                    int B, int C, int D, int ncols, int ncols_p,
                                                                    float* __restrict__ partial) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= ncols_p) return;
  const int S = gridDim.y, sl = blockIdx.y;
  const int b0 = (int)((int64_t)B * sl / S), b1 = (int)((int64_t)B * (sl + 1) / S);
  float acc = 0.f;
  if (j < C * D) {
    const int c = j / D, d = j - c * D;
    for (int b = b0; b < b1; ++b) acc += dlogits[(int64_t)b * C + c] * pooled[(int64_t)b * D + d];
  } else if (j < ncols) {
    const int c = j - C * D;
    for (int b = b0; b < b1; ++b) acc += dlogits[(int64_t)b * C + c];
  }
  partial[(int64_t)sl * ncols_p + j] = acc;
}

int64_t classifier_wgrad_partial_floats(int B, int C, int D) {
  const int S = std::min(B, CLS_WGRAD_SLICES);
  return (int64_t)S * round_up((int64_t)C * D + C, 4);
}

int launch_classifier_head_wgrad(const float* dlogits, const float* pooled, int B, int C, int D, float* partial, float* sum_out,
                                 float* head_grads, hipStream_t s) {
  MAE_REQUIRE(dlogits && pooled && partial && sum_out && head_grads && B > 0 && C > 0 && D > 0, "classifier_head_wgrad: bad arguments");
  const int ncols = C * D + C, ncols_p = (int)round_up(ncols, 4);
  const int S = std::min(B, CLS_WGRAD_SLICES);
  hipLaunchKernelGGL(classifier_head_wgrad_kernel, dim3((unsigned)cdiv(ncols_p, 256), S), dim3(256), 0, s, dlogits, pooled, B, C, D, ncols, ncols_p, partial);
  MAE_LAUNCH_CHECK();
  MAE_TRY(launch_sum_partials(partial, S, ncols_p, sum_out, nullptr, ncols_p, s));
  MAE_HIP(hipMemcpyAsync(head_grads, sum_out, (size_t)ncols * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

// Full-sequence embedding gradient in ONE pass over dres (B, L, D) fp32:
//   dtok (act dtype) = dres with the class-token rows zeroed (the patch-projection weight gradient reads it),
//   partial[slice][t][d] = sum of dres[b, t, d] over the slice's images in ascending order.
// The slices' partials are then added in order: d pos_embed[t] = sum_b dres[b, t], and d cls_token = d pos_embed[0].
// Thread (t, 4 columns) of slice s walks its images with four rows in flight.
// HAS_CLS = false is the patch-only sequence (L = num_patches rows, row t is patch token t + 1): no row is zeroed in dtok.
template <class T, bool HAS_CLS>
__global__ void __launch_bounds__(256) full_grad_split_kernel(const float* __restrict__ dx, int B, int L, int D, T* __restrict__ dtok,
                                                              float* __restrict__ partial) {
  const int D4 = D / 4;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= L * D4) return;
  const int t = q / D4, d = (q - t * D4) * 4;
  const int S = gridDim.y, sl = blockIdx.y;
  const int b0 = (int)((int64_t)B * sl / S), b1 = (int)((int64_t)B * (sl + 1) / S);
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc = z;
  constexpr int U = 4;
  for (int bb = b0; bb < b1; bb += U) {
    f32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t off = (((int64_t)(bb + u) * L + t) * D) + d;
      v[u] = bb + u < b1 ? load4_nt(dx + off) : z;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (bb + u < b1) {
        acc += v[u];
        store4(dtok + (((int64_t)(bb + u) * L + t) * D) + d, HAS_CLS && t == 0 ? z : v[u]);
      }
    }
  }
  store4(partial + (int64_t)sl * L * D + (int64_t)t * D + d, acc);
}

int full_grad_split_slices(int B, int L, int D) {
  const int per_slice = (int)cdiv((int64_t)L * (D / 4), 256);
  return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)B, (int64_t)CLS_EMBED_SLICES, cdiv(2048, per_slice)}));
}

// has_cls = false is the patch-only sequence: the sums land in rows 1..L of dpos ((L + 1) * D floats), and row 0 of dpos and dcls
// (D floats) -- no token carries them -- become exact zeros.  Same slices and summation order either way.
int launch_full_grad_split(const float* dx, int B, int L, int D, int dt, void* dtok, float* dpos, float* dcls, float* partial, bool has_cls,
                           hipStream_t s) {
  const char* who = has_cls ? "full_grad_split" : "patch_grad_split";
  MAE_REQUIRE(dx && dtok && dpos && dcls && partial && B > 0 && L > 0, "%s: bad arguments", who);
  MAE_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1024, "%s: D = %d must be a multiple of 4 in [4, 1024]", who, D);
  MAE_REQUIRE(dt == MAE_F32 || dt == MAE_BF16, "%s: dtype must be MAE_F32 or MAE_BF16 (got %d)", who, dt);
  MAE_REQUIRE((int64_t)B * L < (1ll << 31), "%s: B * L < 2^31", who);
  const int S = full_grad_split_slices(B, L, D);
  const dim3 grid((unsigned)cdiv((int64_t)L * (D / 4), 256), S);
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((has_cls ? full_grad_split_kernel<T, true> : full_grad_split_kernel<T, false>), grid, dim3(256), 0, s, dx, B, L, D, (T*)dtok, partial);
  });
  MAE_LAUNCH_CHECK();
  MAE_TRY(launch_sum_partials(partial, S, L * D, has_cls ? dpos : dpos + D, nullptr, L * D, s));
  if (has_cls) {
    MAE_HIP(hipMemcpyAsync(dcls, dpos, (size_t)D * 4, hipMemcpyDeviceToDevice, s));
  } else {
    MAE_HIP(hipMemsetAsync(dpos, 0, (size_t)D * 4, s));
    MAE_HIP(hipMemsetAsync(dcls, 0, (size_t)D * 4, s));
  }
  return 0;
}

}  // namespace mae

// single-kernel entry (parity tests and reuse): the head's forward and backward on caller features
extern "C" int64_t mae_classifier_head_scratch_bytes(int32_t batch, int32_t num_classes, int32_t dim) {
  if (batch <= 0 || num_classes < 2 || num_classes > mae::HEAD_MAX_CLASSES || dim <= 0) return -1;
  const int64_t B = batch, C = num_classes, D = dim;
  auto seg = [](int64_t n) { return mae::round_up(n, 64); };  // every segment starts 256-byte aligned (vector loads)
  return 4 * (seg(B * D) + seg(B * C) + 2 * seg(B) + seg(mae::classifier_wgrad_partial_floats(batch, num_classes, dim)) + seg(C * D + C));
}

namespace mae {
struct HeadScratch { float *pooled, *dlogits, *row_loss; int32_t* row_correct; float *partial, *hsum; };
static HeadScratch head_scratch(void* scratch, int64_t B, int64_t C, int64_t D) {
  auto seg = [](int64_t n) { return round_up(n, 64); };
  HeadScratch h;
  h.pooled = reinterpret_cast<float*>(scratch);
  h.dlogits = h.pooled + seg(B * D);
  h.row_loss = h.dlogits + seg(B * C);
  h.row_correct = reinterpret_cast<int32_t*>(h.row_loss + seg(B));
  h.partial = h.row_loss + 2 * seg(B);
  h.hsum = h.partial + seg(classifier_wgrad_partial_floats((int)B, (int)C, (int)D));
  return h;
}

// What mae_classifier_head / _ex / _soft add to a HeadCall: the caller's scratch, the packed head (W then bias), the head gradient
// and whether the entry accepts the patch-only sequence and the patch-row mean.  They fill feats .. dfeat_out of `h` themselves.
struct HeadEntry {
  HeadCall h;
  const float* head;
  float* head_grads;
  void* scratch;
  int64_t scratch_bytes;
  bool extended_pools;
};

// The one body of mae_classifier_head / _ex / _soft; soft targets with nothing active launch the hard-label kernels.
static int classifier_head_impl(HeadEntry c, void* stream, const char* who) {
  HeadCall& h = c.h;
  MAE_REQUIRE(h.soft.eps >= 0.f && h.soft.eps < 1.f, "%s: label_smoothing = %g outside [0, 1)", who, (double)h.soft.eps);
  MAE_TRY(check_pool(h.with_cls, h.pool, c.extended_pools, who));
  const bool range = h.range();
  MAE_REQUIRE(h.dt == MAE_F32 || h.dt == MAE_BF16, "%s: dtype must be MAE_F32 or MAE_BF16", who);
  MAE_REQUIRE(!range || h.seq > h.with_cls, "%s: seq_len = %d leaves no patch row to pool", who, h.seq);
  const int64_t need = mae_classifier_head_scratch_bytes(h.B, h.C, h.D);
  MAE_REQUIRE(need > 0 && c.scratch && c.scratch_bytes >= need && ((uintptr_t)c.scratch & 255) == 0,
              "%s: scratch must hold mae_classifier_head_scratch_bytes (%lld) bytes, 256-byte aligned", who, (long long)need);
  MAE_REQUIRE(!h.dfeat_out || c.head_grads, "%s: d_feats needs head_grads", who);
  MAE_REQUIRE(!c.head_grads || h.labels, "%s: gradients need labels", who);
  MAE_REQUIRE(!range || (c.head && (h.labels || (!h.loss_out && !h.correct_out))), "%s: null head, or loss / correct count without labels", who);
  hipStream_t s = (hipStream_t)stream;
  const HeadScratch hs = head_scratch(c.scratch, h.B, h.C, h.D);
  h.W = c.head;
  h.bias = c.head + (int64_t)h.C * h.D;
  h.row_loss = hs.row_loss;
  h.row_correct = hs.row_correct;
  h.pooled_out = c.head_grads ? hs.pooled : nullptr;
  h.dlogits_out = c.head_grads ? hs.dlogits : nullptr;
  MAE_TRY(launch_classifier_head(h, s));
  if (!c.head_grads) return 0;
  return launch_classifier_head_wgrad(hs.dlogits, hs.pooled, h.B, h.C, h.D, hs.partial, hs.hsum, c.head_grads, s);
}
}  // namespace mae

// The three head entries (see mae_hip.h) fill one record each: the first is [cls | patches] with MAE_POOL_CLS or MAE_POOL_MEAN,
// _ex adds with_cls and the patch-row mean, _soft adds the soft targets.  They name their parameters alike:
#define HEAD_ENTRY(c, extended)                                                                                          \
  mae::HeadEntry c{{}, head, head_grads, scratch, scratch_bytes, extended};                                              \
  c.h.feats = feats; c.h.dt = dtype; c.h.B = batch; c.h.seq = seq_len; c.h.D = dim; c.h.pool = pool; c.h.C = num_classes; \
  c.h.labels = labels; c.h.grad_scale = grad_scale; c.h.logits_out = logits; c.h.loss_out = loss_out;                    \
  c.h.correct_out = correct_out; c.h.dfeat_out = d_feats
extern "C" int mae_classifier_head(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t pool,
                                   const float* head, int32_t num_classes, const int64_t* labels, float grad_scale, float* logits,
                                   float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
  HEAD_ENTRY(c, false);
  return mae::classifier_head_impl(c, stream, "mae_classifier_head");
}

extern "C" int mae_classifier_head_ex(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls,
                                      int32_t pool, const float* head, int32_t num_classes, const int64_t* labels, float grad_scale,
                                      float* logits, float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats,
                                      void* scratch, int64_t scratch_bytes, void* stream) {
  HEAD_ENTRY(c, true);
  c.h.with_cls = with_cls;
  return mae::classifier_head_impl(c, stream, "mae_classifier_head_ex");
}

extern "C" int mae_classifier_head_soft(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls,
                                        int32_t pool, const float* head, int32_t num_classes, const int64_t* labels, float grad_scale,
                                        float* logits, float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats,
                                        void* scratch, int64_t scratch_bytes, const int64_t* labels_b, const float* lam,
                                        float label_smoothing, void* stream) {
  HEAD_ENTRY(c, true);
  c.h.with_cls = with_cls;
  c.h.soft = {labels_b, lam, label_smoothing};
  return mae::classifier_head_impl(c, stream, "mae_classifier_head_soft");
}
#undef HEAD_ENTRY

// single-kernel entries (parity tests): the engine-only kernels of this file, see mae_hip.h
extern "C" int64_t mae_full_grad_split_partial_floats(int32_t batch, int32_t seq_len, int32_t dim) {
  if (batch <= 0 || seq_len <= 0 || dim < 4 || dim > 1024 || dim % 4 != 0 || (int64_t)batch * seq_len >= (1ll << 31)) return -1;
  return (int64_t)mae::full_grad_split_slices(batch, seq_len, dim) * seq_len * dim;
}

extern "C" int mae_full_grad_split(const float* dx, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t dtype, void* dtok,
                                   float* dpos, float* dcls, float* partial, void* stream) {
  return mae::launch_full_grad_split(dx, batch, seq_len, dim, dtype, dtok, dpos, dcls, partial, with_cls != 0, (hipStream_t)stream);
}
