// Attention maps of an encoder block: a weighted column sum of the attention probabilities, from the block's saved qkv.
//   P_{b,h}[t, j] = softmax_j(hd^-1/2 q_t . k_j)            S_h[b, j] = sum_t w[b, t] P_{b,h}[t, j]
//   mixed[b, j]   = 1/2 w[b, j] + 1/2 (1 / H) sum_h S_h[b, j]
// w = e_cls gives the class-token map, w = 1 / T the mean attention each key receives, and mixed is one step of attention rollout
// (Abnar & Zuidema 2020): the row r (1/2 mean_h P + 1/2 I) of the row vector r = w.  No T x T matrix is written, V is never read, and the
// saved log-sum-exp is not used: every row is normalised by its own sum.
//
// Geometry.  One workgroup of four waves per image walks the heads in order.  The head's K slice is staged once in LDS as fp32,
// transposed: Kt[d][j] with a row stride of 64 NK + 1 dwords (NK = ceil(T / 64)), so the 64 lanes of a score read, which hold 64
// consecutive keys at one d, hit 64 consecutive banks (a stride of hd dwords would put them all on one at hd = 64).  The staging
// writes, whose lanes hold four consecutive d each at one key, step by four banks: a 2-way conflict on 1 / T of the traffic.
// Wave v takes the groups of four consecutive query rows 4 v, 4 (v + 4), ... in order; lane l owns the keys l, l + 64, ... (NK of them,
// in registers).  A row is one coalesced load of q (lane d holds q[d]), hd v_readlane broadcasts, hd NK fused multiply-adds per lane
// in the order of d, the wave's maximum and sum by the xor butterfly, one division w / l, and NK fused multiply-adds into the lane's
// column sums, the rows of a group in order.  The four rows of a group share every key read, so the inner loop is bound by its
// multiply-adds and not by the LDS.  A row whose weight is exactly zero is skipped and its q is not read (the branches are uniform:
// a wave owns the row), a group of four such rows before anything is computed: a one-hot w costs one group per head.  The four waves' column sums meet in LDS and are added in wave order, the heads in head order: every
// order is fixed by the shape, there are no atomics, and an image's result does not depend on its batch.
#include "kernels.h"

namespace mae {

constexpr int AC_THREADS = 256;
constexpr int AC_WAVES = AC_THREADS / 64;
constexpr int AC_ROWS = 4;                 // query rows of a group: one read of a key from LDS serves all four
constexpr int AC_MAX_NK = 8;               // key registers of a lane: T <= 512
constexpr int AC_LDS_BYTES = 160 * 1024;

static size_t colsum_lds_bytes(int hd, int nk) { return ((size_t)hd * (64 * nk + 1) + (size_t)AC_WAVES * 64 * nk) * sizeof(float); }

// the largest T whose layout fits: NK key registers per lane, and Kt plus the four waves' column sums in the CU's LDS
int attention_colsum_max_tokens(int hd, int dt) {
  if ((dt != MAE_F32 && dt != MAE_BF16) || (hd != 16 && hd != 24 && hd != 32 && hd != 48 && hd != 64)) return -1;
  int nk = AC_MAX_NK;
  while (nk > 1 && colsum_lds_bytes(hd, nk) > (size_t)AC_LDS_BYTES) --nk;
  return 64 * nk;
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ float uniform_value(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}

// LDS: Kt[hd][64 NK + 1], then acc[4][64 NK]
template <class T, int NK>
__global__ void __launch_bounds__(AC_THREADS) attn_colsum_kernel(const T* __restrict__ qkv, const float* __restrict__ w, int Tn, int H, int hd,
                                                                 float scale, float half_inv_h, float* __restrict__ per_head,
                                                                 int64_t per_head_stride, float* __restrict__ mixed) {
  extern __shared__ __attribute__((aligned(16))) float ac_lds[];
  constexpr int TP = 64 * NK, KS = TP + 1;
  constexpr int NJ = (TP + AC_THREADS - 1) / AC_THREADS;   // keys a thread folds: j = thread + 256 i
  float* Kt = ac_lds;
  float* accL = ac_lds + hd * KS;
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int b = blockIdx.x, hd4 = hd >> 2;
  const int rs = 3 * H * hd;
  const T* base = qkv + (int64_t)b * Tn * rs;
  const float* wb = w + (int64_t)b * Tn;
  float hsum[NJ];
#pragma unroll
  for (int i = 0; i < NJ; ++i) hsum[i] = 0.f;
  for (int h = 0; h < H; ++h) {
    __syncthreads();   // the previous head's scores and fold have been read
    for (int i = threadIdx.x; i < Tn * hd4; i += AC_THREADS) {
      const int j = i / hd4, d = (i - j * hd4) * 4;
      const f32x4 v = load4(base + j * rs + (H + h) * hd + d);
#pragma unroll
      for (int e = 0; e < 4; ++e) Kt[(d + e) * KS + j] = v[e];
    }
    __syncthreads();
    float acc[NK];
#pragma unroll
    for (int c = 0; c < NK; ++c) acc[c] = 0.f;
    for (int t0 = AC_ROWS * wv; t0 < Tn; t0 += AC_ROWS * AC_WAVES) {
      float wt[AC_ROWS], qv[AC_ROWS];
      bool any = false;
#pragma unroll
      for (int r = 0; r < AC_ROWS; ++r) {
        wt[r] = t0 + r < Tn ? uniform_value(wb[t0 + r]) : 0.f;
        any |= wt[r] != 0.f;
      }
      if (!any) continue;   // the group contributes nothing
#pragma unroll
      for (int r = 0; r < AC_ROWS; ++r)   // a row of weight zero is skipped below: its q is not read
        qv[r] = (wt[r] != 0.f && lane < hd) ? to_f(base[(t0 + r) * rs + h * hd + lane]) : 0.f;
      float s[AC_ROWS][NK];
#pragma unroll
      for (int r = 0; r < AC_ROWS; ++r)
#pragma unroll
        for (int c = 0; c < NK; ++c) s[r][c] = 0.f;
#pragma unroll 4
      for (int d = 0; d < hd; ++d) {
        const float* kr = Kt + d * KS + lane;
        float kk[NK];
#pragma unroll
        for (int c = 0; c < NK; ++c) kk[c] = kr[64 * c];
#pragma unroll
        for (int r = 0; r < AC_ROWS; ++r) {
          const float qd = lane_value(qv[r], d);
#pragma unroll
          for (int c = 0; c < NK; ++c) s[r][c] = fmaf(qd, kk[c], s[r][c]);
        }
      }
#pragma unroll
      for (int r = 0; r < AC_ROWS; ++r) {
        if (wt[r] == 0.f) continue;
        float m = -INFINITY;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
          s[r][c] = lane + 64 * c < Tn ? s[r][c] * scale : -INFINITY;   // the slots past T hold whatever the LDS held
          m = fmaxf(m, s[r][c]);
        }
        m = wave_max(m);   // key 0 exists: finite
        float l = 0.f;
#pragma unroll
        for (int c = 0; c < NK; ++c) {
          s[r][c] = __expf(s[r][c] - m);   // 0 for a slot past T
          l += s[r][c];
        }
        l = wave_sum(l);   // >= 1: the row's maximum gives exp(0)
        const float coef = wt[r] / l;
#pragma unroll
        for (int c = 0; c < NK; ++c) acc[c] = fmaf(coef, s[r][c], acc[c]);
      }
    }
#pragma unroll
    for (int c = 0; c < NK; ++c) accL[wv * TP + lane + 64 * c] = acc[c];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      const int j = threadIdx.x + AC_THREADS * i;
      if (j < Tn) {
        const float v = ((accL[j] + accL[TP + j]) + accL[2 * TP + j]) + accL[3 * TP + j];
        if (per_head) per_head[(int64_t)b * per_head_stride + (int64_t)h * Tn + j] = v;
        hsum[i] += v;
      }
    }
  }
  if (mixed) {
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
      const int j = threadIdx.x + AC_THREADS * i;
      if (j < Tn) mixed[(int64_t)b * Tn + j] = fmaf(half_inv_h, hsum[i], 0.5f * wb[j]);
    }
  }
}

// start weights of a map: row `row` of the identity (the class query is row 0), or 1 / T in every column for row < 0
__global__ void __launch_bounds__(256) attn_weight_fill_kernel(float* __restrict__ w, int64_t n, int Tn, int row, float uniform) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) w[i] = row < 0 ? uniform : (i % Tn == row ? 1.f : 0.f);
}

int launch_attention_weight_fill(float* w, int B, int T, int row, hipStream_t s) {
  MAE_REQUIRE(w && B > 0 && T > 0 && row < T, "attention_weight_fill: bad arguments");
  const int64_t n = (int64_t)B * T;
  MAE_REQUIRE(n < (1ll << 31), "attention_weight_fill: batch * T = %lld must stay below 2^31", (long long)n);
  hipLaunchKernelGGL(attn_weight_fill_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, s, w, n, T, row, 1.0f / (float)T);
  MAE_LAUNCH_CHECK();
  return 0;
}

template <class T, int NK>
static int run_colsum(const void* qkv, int B, int Tn, int H, int hd, const float* w, float* per_head, int64_t stride, float* mixed, hipStream_t s) {
  auto kern = attn_colsum_kernel<T, NK>;
  const size_t lds = colsum_lds_bytes(hd, NK);
  MAE_TRY(allow_lds(kern, lds));
  hipLaunchKernelGGL(kern, dim3((unsigned)B), dim3(AC_THREADS), lds, s, (const T*)qkv, w, Tn, H, hd, 1.0f / sqrtf((float)hd), 0.5f / (float)H, per_head,
                     stride, mixed);
  MAE_LAUNCH_CHECK();
  return 0;
}

static bool ranges_overlap(const void* a, const void* b, int64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + (uintptr_t)bytes && y < x + (uintptr_t)bytes;
}

int launch_attention_colsum(const void* qkv, int dt, int B, int T, int H, int hd, const float* w, float* per_head, int64_t per_head_stride,
                            float* mixed, hipStream_t s) {
  const char* who = "attention_colsum";
  MAE_REQUIRE(qkv && w, "%s: null qkv / row_weight", who);
  MAE_REQUIRE(per_head || mixed, "%s: per_head and mixed are both null", who);
  MAE_REQUIRE(dt == MAE_F32 || dt == MAE_BF16, "%s: bad dtype %d", who, dt);
  MAE_REQUIRE(hd == 16 || hd == 24 || hd == 32 || hd == 48 || hd == 64, "%s: head_dim %d unsupported (16, 24, 32, 48, 64)", who, hd);
  MAE_REQUIRE(H >= 1 && H <= 16, "%s: H = %d outside [1, 16]", who, H);
  MAE_REQUIRE(B >= 1 && T >= 1, "%s: batch %d / T %d must be positive", who, B, T);
  MAE_REQUIRE((int64_t)B * T < (1ll << 31), "%s: batch * T = %lld must stay below 2^31", who, (long long)B * T);
  const int max_t = attention_colsum_max_tokens(hd, dt);
  MAE_REQUIRE(T <= max_t, "%s: T = %d is beyond the %d tokens whose keys fit the LDS layout at head_dim %d", who, T, max_t, hd);
  MAE_REQUIRE(((uintptr_t)qkv & 15) == 0 && ((uintptr_t)w & 15) == 0 && ((uintptr_t)mixed & 15) == 0 && ((uintptr_t)per_head & 3) == 0,
              "%s: qkv, row_weight and mixed must be 16-byte aligned, per_head 4-byte", who);
  if (per_head) MAE_REQUIRE(per_head_stride >= (int64_t)H * T, "%s: per_head_stride = %lld below H * T = %lld", who, (long long)per_head_stride, (long long)H * T);
  if (mixed) MAE_REQUIRE(!ranges_overlap(mixed, w, (int64_t)B * T * 4), "%s: mixed must not alias row_weight", who);
  int r = 1;
  with_dtype(dt, [&](auto t) {
    using E = decltype(t);
    switch (cdiv(T, 64)) {
      case 1: r = run_colsum<E, 1>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
      case 2: r = run_colsum<E, 2>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
      case 3: r = run_colsum<E, 3>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
      case 4: r = run_colsum<E, 4>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
      case 5: r = run_colsum<E, 5>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
      default: r = run_colsum<E, AC_MAX_NK>(qkv, B, T, H, hd, w, per_head, per_head_stride, mixed, s); break;
    }
  });
  return r;
}

}  // namespace mae

extern "C" int32_t mae_attention_colsum_max_tokens(int32_t hd, int32_t dtype) { return mae::attention_colsum_max_tokens(hd, dtype); }

extern "C" int mae_attention_colsum(const void* qkv, int32_t dtype, int32_t batch, int32_t T, int32_t H, int32_t hd, const float* row_weight,
                                    float* per_head, int64_t per_head_stride, float* mixed, void* stream) {
  return mae::launch_attention_colsum(qkv, dtype, batch, T, H, hd, row_weight, per_head, per_head_stride, mixed, (hipStream_t)stream);
}
