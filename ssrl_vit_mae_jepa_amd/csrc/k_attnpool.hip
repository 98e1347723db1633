// The attentive probe on cached patch tokens: one learned query cross-attends over the frozen tokens of an image,
// a linear layer classifies the pooled vector.  No reference counterpart; the definition is AIM's attention-pooling classifier
// with one query behind BatchNorm1d(affine=False):
//   xh = (x - mu) rstd;  k, v = xh Wk^T, xh Wv^T;  s[b,t,h] = hd^-1/2 q[h] . k[b,t,h];  a = softmax_t s;  p[b,h] = sum_t a v[b,t,h]
// What runs is the folded form, which never writes anything of the size of x and reads x once per pass:
//   Uq[h] = rstd * (hd^-1/2 Wk[h]^T q[h])          s = (x - mu) . Uq[h]           ybar[b,h] = sum_t a (x - mu)
//   p[b,h] = Wv[h] (rstd * ybar[b,h])
//   G[b,h] = rstd * (Wv[h]^T dp[b,h])              delta = ybar . G               da = (x - mu) . G            ds = a (da - delta)
//   dUq[h] = sum_{b,t} ds (x - mu)                 dWv[h] = rstd * sum_b dp[b,h] (x) ybar[b,h]
//   dWk[h] = hd^-1/2 q[h] (x) (rstd * dUq[h])      dq[h]  = hd^-1/2 Wk[h] (rstd * dUq[h])
// Every sum has a fixed order that depends on the shape alone; there are no atomics.
//
// Pool geometry.  A workgroup of four waves owns one image (forward) or a contiguous run of images (backward).  A lane holds the
// float4 columns lane + 64 i (i < NV = ceil(D / 256)) of a token row, so a wave reads a row as whole 1 KiB segments straight into
// registers.  The heads are dealt to HG = 1 / 2 / 4 groups of HPW = ceil(H / HG) <= 4 heads (H <= 4 / <= 8 / <= 16); the TS = 4 / HG
// waves of a group split the tokens in chunks: wave tsi takes the chunks tsi, tsi + TS, ...  A wave keeps Uq (and G) of its heads and
// its accumulators in registers: HPW NV float4 each.  The waves of a group are merged through LDS in the order of tsi.
#include "kernels.h"

namespace mae {

constexpr int AP_FWD_TC = 4;        // token rows a wave holds per trip of the forward walk
constexpr int AP_BWD_TC = 2;        // ... of the backward walk (it also keeps G)
constexpr int AP_BWD_SLOTS = 512;   // image slices of the backward: partial[slot][H][D], added by launch_sum_partials
constexpr int AP_IMG_TILE = 8;      // images that share one read of a weight row in the two projections
constexpr int AP_WV_SLICES = 8;     // batch slices of the dWv partials

struct ApGeo {
  int nv, hg, hpw, ts;
};
static ApGeo ap_geometry(int D, int H) {
  ApGeo g;
  g.nv = (int)cdiv(D / 4, 64);
  g.hg = H <= 4 ? 1 : H <= 8 ? 2 : 4;
  g.hpw = (int)cdiv(H, g.hg);
  g.ts = 4 / g.hg;
  return g;
}

__device__ __forceinline__ float dot4_acc(f32x4 a, f32x4 b, float acc) {
  return fmaf(a[3], b[3], fmaf(a[2], b[2], fmaf(a[1], b[1], fmaf(a[0], b[0], acc))));
}

// one lane's columns of the HPW head rows of a (H, D) matrix that start at head h0; heads past H and columns past D read as zeros
template <int NV, int HPW>
__device__ __forceinline__ void ap_load_heads(const float* __restrict__ m, int h0, int H, int D, int lane, f32x4 (&out)[HPW][NV]) {
  const int D4 = D >> 2;
#pragma unroll
  for (int h = 0; h < HPW; ++h)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      out[h][i] = (h0 + h < H && c < D4) ? load4(m + (int64_t)(h0 + h) * D + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// TC token rows t0 .. t0 + TC of one image, centred; rows past T and columns past D read as zeros
template <int NV, int TC>
__device__ __forceinline__ void ap_load_tokens(const float* __restrict__ xb, int t0, int T, int D, int lane, const f32x4 (&mu)[NV],
                                               f32x4 (&v)[TC][NV]) {
  const int D4 = D >> 2;
#pragma unroll
  for (int j = 0; j < TC; ++j)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      v[j][i] = (t0 + j < T && c < D4) ? load4(xb + (int64_t)(t0 + j) * D + c * 4) - mu[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

template <int NV>
__device__ __forceinline__ float ap_row_dot(const f32x4 (&a)[NV], const f32x4 (&b)[NV]) {
  float p = 0.f;
#pragma unroll
  for (int i = 0; i < NV; ++i) p = dot4_acc(a[i], b[i], p);
  return wave_sum(p);  // the xor butterfly: every lane ends with the same bits
}

// LDS: acc[4][HPW][D] floats, then m[4][HPW], then l[4][HPW]
template <int NV, int HPW>
__global__ void __launch_bounds__(256) attn_pool_fwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ uq, int T, int D, int H, int ts,
                                                            float* __restrict__ ybar, float* __restrict__ lse) {
  extern __shared__ __attribute__((aligned(16))) float ap_lds[];
  constexpr int TC = AP_FWD_TC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, D4 = D >> 2;
  const int grp = w / ts, tsi = w - grp * ts, h0 = grp * HPW;
  const float* xb = x + (int64_t)blockIdx.x * T * D;
  f32x4 mu[NV], u[HPW][NV], acc[HPW][NV];
  float m[HPW], l[HPW];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    mu[i] = (mean && c < D4) ? load4(mean + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ap_load_heads<NV, HPW>(uq, h0, H, D, lane, u);
#pragma unroll
  for (int h = 0; h < HPW; ++h) {
    m[h] = -INFINITY;
    l[h] = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[h][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int t0 = tsi * TC; t0 < T; t0 += ts * TC) {  // the first row of a chunk always exists: the new maximum is finite
    f32x4 v[TC][NV];
    ap_load_tokens<NV, TC>(xb, t0, T, D, lane, mu, v);
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
      float s[TC], mn = m[h];
#pragma unroll
      for (int j = 0; j < TC; ++j) {
        s[j] = t0 + j < T ? ap_row_dot<NV>(v[j], u[h]) : -INFINITY;
        mn = fmaxf(mn, s[j]);
      }
      const float sc = expf(m[h] - mn);  // 0 on the first chunk
      l[h] *= sc;
#pragma unroll
      for (int i = 0; i < NV; ++i) acc[h][i] *= sc;
#pragma unroll
      for (int j = 0; j < TC; ++j) {
        const float p = expf(s[j] - mn);   // 0 for a row past T
        l[h] += p;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[h][i] += v[j][i] * p;
      }
      m[h] = mn;
    }
  }
  float* accL = ap_lds;
  float* mL = ap_lds + 4 * HPW * D;
  float* lL = mL + 4 * HPW;
#pragma unroll
  for (int h = 0; h < HPW; ++h) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) store4(accL + (w * HPW + h) * D + c * 4, acc[h][i]);
    }
    if (lane == 0) {
      mL[w * HPW + h] = m[h];
      lL[w * HPW + h] = l[h];
    }
  }
  __syncthreads();
  // merge the token splits of a head in the order of tsi: a wave that saw no token has m = -inf, l = 0 and weighs exp(-inf) = 0
  for (int idx = threadIdx.x; idx < H * D4; idx += 256) {
    const int h = idx / D4, c = idx - h * D4;
    const int g = h / HPW, hl = h - g * HPW;
    float M = -INFINITY;
    for (int i = 0; i < ts; ++i) M = fmaxf(M, mL[(g * ts + i) * HPW + hl]);
    float L = 0.f;
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < ts; ++i) {
      const int slot = (g * ts + i) * HPW + hl;
      const float wgt = expf(mL[slot] - M);
      L += lL[slot] * wgt;
      a += load4(accL + slot * D + c * 4) * wgt;
    }
    store4(ybar + ((int64_t)blockIdx.x * H + h) * D + c * 4, a / L);
    if (c == 0) lse[(int64_t)blockIdx.x * H + h] = M + logf(L);
  }
}

// LDS: acc[4][HPW][D] floats.  Block blk walks the images [blk ipb, min(B, (blk + 1) ipb)) in order.
template <int NV, int HPW>
__global__ void __launch_bounds__(256) attn_pool_bwd_kernel(const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ uq, const float* __restrict__ lse,
                                                            const float* __restrict__ ybar, const float* __restrict__ g, int B, int T,
                                                            int D, int H, int ts, int ipb, float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float ap_lds[];
  constexpr int TC = AP_BWD_TC;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, D4 = D >> 2;
  const int grp = w / ts, tsi = w - grp * ts, h0 = grp * HPW;
  f32x4 mu[NV], u[HPW][NV], acc[HPW][NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    mu[i] = (mean && c < D4) ? load4(mean + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ap_load_heads<NV, HPW>(uq, h0, H, D, lane, u);
#pragma unroll
  for (int h = 0; h < HPW; ++h)
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[h][i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int b_lo = blockIdx.x * ipb, b_hi = b_lo + ipb < B ? b_lo + ipb : B;
  for (int b = b_lo; b < b_hi; ++b) {
    const float* xb = x + (int64_t)b * T * D;
    f32x4 gg[HPW][NV];
    float delta[HPW], ls[HPW];
    ap_load_heads<NV, HPW>(g + (int64_t)b * H * D, h0, H, D, lane, gg);
    {
      f32x4 yb[HPW][NV];
      ap_load_heads<NV, HPW>(ybar + (int64_t)b * H * D, h0, H, D, lane, yb);
#pragma unroll
      for (int h = 0; h < HPW; ++h) {
        delta[h] = ap_row_dot<NV>(yb[h], gg[h]);
        ls[h] = h0 + h < H ? lse[(int64_t)b * H + h0 + h] : 0.f;
      }
    }
    for (int t0 = tsi * TC; t0 < T; t0 += ts * TC) {
      f32x4 v[TC][NV];
      ap_load_tokens<NV, TC>(xb, t0, T, D, lane, mu, v);
#pragma unroll
      for (int h = 0; h < HPW; ++h)
#pragma unroll
        for (int j = 0; j < TC; ++j) {
          const float s = ap_row_dot<NV>(v[j], u[h]);
          const float da = ap_row_dot<NV>(v[j], gg[h]);
          const float ds = t0 + j < T ? expf(s - ls[h]) * (da - delta[h]) : 0.f;
#pragma unroll
          for (int i = 0; i < NV; ++i) acc[h][i] += v[j][i] * ds;
        }
    }
  }
#pragma unroll
  for (int h = 0; h < HPW; ++h)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) store4(ap_lds + (w * HPW + h) * D + c * 4, acc[h][i]);
    }
  __syncthreads();
  for (int idx = threadIdx.x; idx < H * D4; idx += 256) {
    const int h = idx / D4, c = idx - h * D4;
    const int gr = h / HPW, hl = h - gr * HPW;
    f32x4 a = load4(ap_lds + ((gr * ts) * HPW + hl) * D + c * 4);
    for (int i = 1; i < ts; ++i) a += load4(ap_lds + ((gr * ts + i) * HPW + hl) * D + c * 4);
    store4(partial + ((int64_t)blockIdx.x * H + h) * D + c * 4, a);
  }
}

// f(int_c<NV>, int_c<HPW>) for the geometry's register shape
template <int N>
struct ap_int {
  static constexpr int value = N;
};
template <class F>
static void with_ap_shape(const ApGeo& g, F&& f) {
  const auto hp = [&](auto nv) {
    switch (g.hpw) {
      case 1: f(nv, ap_int<1>{}); break;
      case 2: f(nv, ap_int<2>{}); break;
      case 3: f(nv, ap_int<3>{}); break;
      default: f(nv, ap_int<4>{}); break;
    }
  };
  switch (g.nv) {
    case 1: hp(ap_int<1>{}); break;
    case 2: hp(ap_int<2>{}); break;
    case 3: hp(ap_int<3>{}); break;
    default: hp(ap_int<4>{}); break;
  }
}

static bool ap_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the limits every entry point of this file shares; B * T is checked where there is a T
static int ap_check_shape(int64_t B, int64_t T, int D, int H, const char* who) {
  MAE_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1024, "%s: dim %d must be a multiple of 4 in [4, 1024]", who, D);
  MAE_REQUIRE(H >= 1 && H <= 16 && D % H == 0, "%s: heads = %d must be in [1, 16] and divide dim %d", who, H, D);
  MAE_REQUIRE(B >= 1 && T >= 1, "%s: batch %lld and tokens %lld must be positive", who, (long long)B, (long long)T);
  MAE_REQUIRE(B < ((int64_t)1 << 31) && T < ((int64_t)1 << 31) && B * T < ((int64_t)1 << 31), "%s: batch * tokens = %lld * %lld must stay below 2^31",
              who, (long long)B, (long long)T);
  return 0;
}
static bool ap_shape_ok(int64_t B, int64_t T, int D, int H) {
  return D % 4 == 0 && D >= 4 && D <= 1024 && H >= 1 && H <= 16 && D % H == 0 && B >= 1 && T >= 1 && B < ((int64_t)1 << 31) &&
         T < ((int64_t)1 << 31) && B * T < ((int64_t)1 << 31);
}

int launch_attn_pool_fwd(const float* x, const float* mean, const float* uq, int64_t B, int64_t T, int D, int H, float* ybar, float* lse,
                         hipStream_t s) {
  const char* who = "attn_pool_fwd";
  MAE_TRY(ap_check_shape(B, T, D, H, who));
  MAE_REQUIRE(x && uq && ybar && lse, "%s: x / uq / ybar / lse is null", who);
  MAE_REQUIRE(ap_aligned16(x) && ap_aligned16(mean) && ap_aligned16(uq) && ap_aligned16(ybar) && ap_aligned16(lse),
              "%s: every buffer must be 16-byte aligned", who);
  const ApGeo g = ap_geometry(D, H);
  const size_t lds = ((size_t)4 * g.hpw * D + 8 * g.hpw) * sizeof(float);
  int rc = 0;
  with_ap_shape(g, [&](auto nv, auto hpw) {
    auto kernel = attn_pool_fwd_kernel<decltype(nv)::value, decltype(hpw)::value>;
    rc = allow_lds(kernel, lds);
    if (rc) return;
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(256), lds, s, x, mean, uq, (int)T, D, H, g.ts, ybar, lse);
  });
  MAE_TRY(rc);
  MAE_LAUNCH_CHECK();
  return 0;
}

static int ap_bwd_images_per_block(int64_t B) { return (int)cdiv(B, AP_BWD_SLOTS); }

int64_t attn_pool_bwd_scratch_bytes(int64_t B, int64_t T, int D, int H) {
  if (!ap_shape_ok(B, T, D, H)) return -1;
  return cdiv(B, ap_bwd_images_per_block(B)) * H * D * (int64_t)sizeof(float);
}

int launch_attn_pool_bwd(const float* x, const float* mean, const float* uq, const float* lse, const float* ybar, const float* g, int64_t B,
                         int64_t T, int D, int H, float* duq, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  const char* who = "attn_pool_bwd";
  MAE_TRY(ap_check_shape(B, T, D, H, who));
  MAE_REQUIRE(x && uq && lse && ybar && g && duq, "%s: x / uq / lse / ybar / g / duq is null", who);
  MAE_REQUIRE(ap_aligned16(x) && ap_aligned16(mean) && ap_aligned16(uq) && ap_aligned16(lse) && ap_aligned16(ybar) && ap_aligned16(g) &&
              ap_aligned16(duq) && ap_aligned16(scratch), "%s: every buffer must be 16-byte aligned", who);
  const int64_t need = attn_pool_bwd_scratch_bytes(B, T, D, H);
  MAE_REQUIRE(scratch && scratch_bytes >= need, "%s: scratch_bytes = %lld, mae_attn_pool_bwd_scratch_bytes asks for %lld", who,
              (long long)scratch_bytes, (long long)need);
  const ApGeo geo = ap_geometry(D, H);
  const int ipb = ap_bwd_images_per_block(B), grid = (int)cdiv(B, ipb);
  const size_t lds = (size_t)4 * geo.hpw * D * sizeof(float);
  int rc = 0;
  with_ap_shape(geo, [&](auto nv, auto hpw) {
    auto kernel = attn_pool_bwd_kernel<decltype(nv)::value, decltype(hpw)::value>;
    rc = allow_lds(kernel, lds);
    if (rc) return;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, x, mean, uq, lse, ybar, g, (int)B, (int)T, D, H, geo.ts, ipb, (float*)scratch);
  });
  MAE_TRY(rc);
  MAE_LAUNCH_CHECK();
  return launch_sum_partials((const float*)scratch, grid, H * D, duq, nullptr, H * D, s);
}

// ---------------------------------------------------------------------------------------------------
// The small pieces: at most about B D^2 flops, plain fp32, one wave per output row or one thread per float4 column
// ---------------------------------------------------------------------------------------------------
// uq[h][d] = rstd[d] * (scale * sum_j q[h hd + j] Wk[h hd + j][d]), j ascending
__global__ void __launch_bounds__(256) ap_fold_kernel(const float* __restrict__ q, const float* __restrict__ wk, const float* __restrict__ rstd,
                                                      int D, int H, float scale, float* __restrict__ uq) {
  const int D4 = D >> 2, hd = D / H;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= H * D4) return;
  const int h = idx / D4, c = idx - h * D4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < hd; ++j) acc += load4(wk + (int64_t)(h * hd + j) * D + c * 4) * q[h * hd + j];
  store4(uq + (int64_t)h * D + c * 4, load4(rstd + c * 4) * (acc * scale));
}

// one wave per weight row n = h hd + j and tile of AP_IMG_TILE images: p[b][n] = sum_d Wv[n][d] (rstd[d] ybar[b][h][d])
__global__ void __launch_bounds__(256) ap_project_kernel(const float* __restrict__ ybar, const float* __restrict__ rstd,
                                                         const float* __restrict__ wv, int B, int D, int H, float* __restrict__ p) {
  const int lane = threadIdx.x & 63, D4 = D >> 2, hd = D / H;
  const int64_t wid = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = (int)(wid % D), b0 = (int)(wid / D) * AP_IMG_TILE;
  if (b0 >= B) return;
  const int h = n / hd;
  f32x4 wr[4];  // Wv[n] * rstd, this lane's columns
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    wr[i] = c < D4 ? load4(wv + (int64_t)n * D + c * 4) * load4(rstd + c * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int b = b0; b < b0 + AP_IMG_TILE && b < B; ++b) {
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) acc = dot4_acc(load4(ybar + ((int64_t)b * H + h) * D + c * 4), wr[i], acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) p[(int64_t)b * D + n] = acc;
  }
}

// one thread per (tile of AP_IMG_TILE images, head, float4 column): G[b][h][d] = rstd[d] sum_j dp[b][h hd + j] Wv[h hd + j][d], j ascending
__global__ void __launch_bounds__(256) ap_project_dgrad_kernel(const float* __restrict__ dp, const float* __restrict__ rstd,
                                                               const float* __restrict__ wv, int B, int D, int H, float* __restrict__ g) {
  const int D4 = D >> 2, hd = D / H;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t tiles = (B + AP_IMG_TILE - 1) / AP_IMG_TILE;
  if (idx >= tiles * H * D4) return;
  const int c = (int)(idx % D4), h = (int)((idx / D4) % H), b0 = (int)(idx / ((int64_t)D4 * H)) * AP_IMG_TILE;
  f32x4 acc[AP_IMG_TILE];
#pragma unroll
  for (int k = 0; k < AP_IMG_TILE; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < hd; ++j) {
    const f32x4 wrow = load4(wv + (int64_t)(h * hd + j) * D + c * 4);
#pragma unroll
    for (int k = 0; k < AP_IMG_TILE; ++k)
      if (b0 + k < B) acc[k] += wrow * dp[(int64_t)(b0 + k) * D + h * hd + j];
  }
  const f32x4 r = load4(rstd + c * 4);
#pragma unroll
  for (int k = 0; k < AP_IMG_TILE; ++k)
    if (b0 + k < B) store4(g + ((int64_t)(b0 + k) * H + h) * D + c * 4, r * acc[k]);
}

// one thread per (batch slice, weight row n, float4 column): partial[slice][n][d] = sum over the slice's images, b ascending, of
// dp[b][n] ybar[b][h][d]
__global__ void __launch_bounds__(256) ap_project_wgrad_kernel(const float* __restrict__ dp, const float* __restrict__ ybar, int B, int D, int H,
                                                               int per_slice, float* __restrict__ partial) {
  const int D4 = D >> 2, hd = D / H;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)D * D4) return;
  const int c = (int)(idx % D4), n = (int)(idx / D4), h = n / hd;
  const int b_lo = blockIdx.y * per_slice, b_hi = b_lo + per_slice < B ? b_lo + per_slice : B;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int b = b_lo; b < b_hi; ++b) acc += load4(ybar + ((int64_t)b * H + h) * D + c * 4) * dp[(int64_t)b * D + n];
  store4(partial + ((int64_t)blockIdx.y * D + n) * D + c * 4, acc);
}

// dwv *= rstd per column, in place on the summed partials
__global__ void __launch_bounds__(256) ap_scale_columns_kernel(float* __restrict__ m, const float* __restrict__ rstd, int D) {
  const int D4 = D >> 2;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)D * D4) return;
  const int c = (int)(idx % D4);
  store4(m + idx * 4, load4(m + idx * 4) * load4(rstd + c * 4));
}

// one wave per weight row n = h hd + j: dU = rstd dUq[h]; dWk[n] = (scale q[n]) dU; dq[n] = scale sum_d Wk[n][d] dU[d]
__global__ void __launch_bounds__(256) ap_fold_bwd_kernel(const float* __restrict__ duq, const float* __restrict__ q, const float* __restrict__ wk,
                                                          const float* __restrict__ rstd, int D, int H, float scale, float* __restrict__ dq,
                                                          float* __restrict__ dwk) {
  const int lane = threadIdx.x & 63, D4 = D >> 2, hd = D / H;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= D) return;
  const int h = n / hd;
  const float qs = scale * q[n];
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      const f32x4 du = load4(rstd + c * 4) * load4(duq + (int64_t)h * D + c * 4);
      store4(dwk + (int64_t)n * D + c * 4, du * qs);
      acc = dot4_acc(load4(wk + (int64_t)n * D + c * 4), du, acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) dq[n] = scale * acc;
}

static float ap_scale(int D, int H) { return 1.0f / sqrtf((float)(D / H)); }

int launch_attn_probe_fold(const float* q, const float* wk, const float* rstd, int D, int H, float* uq, hipStream_t s) {
  const char* who = "attn_probe_fold";
  MAE_TRY(ap_check_shape(1, 1, D, H, who));
  MAE_REQUIRE(q && wk && rstd && uq, "%s: q / wk / rstd / uq is null", who);
  MAE_REQUIRE(ap_aligned16(q) && ap_aligned16(wk) && ap_aligned16(rstd) && ap_aligned16(uq), "%s: every buffer must be 16-byte aligned", who);
  hipLaunchKernelGGL(ap_fold_kernel, dim3((unsigned)cdiv(H * (D / 4), 256)), dim3(256), 0, s, q, wk, rstd, D, H, ap_scale(D, H), uq);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_attn_probe_fold_bwd(const float* duq, const float* q, const float* wk, const float* rstd, int D, int H, float* dq, float* dwk,
                               hipStream_t s) {
  const char* who = "attn_probe_fold_bwd";
  MAE_TRY(ap_check_shape(1, 1, D, H, who));
  MAE_REQUIRE(duq && q && wk && rstd && dq && dwk, "%s: duq / q / wk / rstd / dq / dwk is null", who);
  MAE_REQUIRE(ap_aligned16(duq) && ap_aligned16(q) && ap_aligned16(wk) && ap_aligned16(rstd) && ap_aligned16(dq) && ap_aligned16(dwk),
              "%s: every buffer must be 16-byte aligned", who);
  hipLaunchKernelGGL(ap_fold_bwd_kernel, dim3((unsigned)cdiv(D, 4)), dim3(256), 0, s, duq, q, wk, rstd, D, H, ap_scale(D, H), dq, dwk);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_attn_probe_project(const float* ybar, const float* rstd, const float* wv, int64_t B, int D, int H, float* p, hipStream_t s) {
  const char* who = "attn_probe_project";
  MAE_TRY(ap_check_shape(B, 1, D, H, who));
  MAE_REQUIRE(ybar && rstd && wv && p, "%s: ybar / rstd / wv / p is null", who);
  MAE_REQUIRE(ap_aligned16(ybar) && ap_aligned16(rstd) && ap_aligned16(wv) && ap_aligned16(p), "%s: every buffer must be 16-byte aligned", who);
  const int64_t waves = cdiv(B, AP_IMG_TILE) * D;
  hipLaunchKernelGGL(ap_project_kernel, dim3((unsigned)cdiv(waves, 4)), dim3(256), 0, s, ybar, rstd, wv, (int)B, D, H, p);
  MAE_LAUNCH_CHECK();
  return 0;
}

static int ap_wv_slices(int64_t B) { return (int)std::min<int64_t>(cdiv(B, 64), AP_WV_SLICES); }

int64_t attn_probe_project_bwd_scratch_bytes(int64_t B, int D, int H) {
  if (!ap_shape_ok(B, 1, D, H)) return -1;
  return (int64_t)ap_wv_slices(B) * D * D * (int64_t)sizeof(float);
}

int launch_attn_probe_project_bwd(const float* dp, const float* ybar, const float* rstd, const float* wv, int64_t B, int D, int H, float* g,
                                  float* dwv, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  const char* who = "attn_probe_project_bwd";
  MAE_TRY(ap_check_shape(B, 1, D, H, who));
  MAE_REQUIRE(dp && ybar && rstd && wv && g && dwv, "%s: dp / ybar / rstd / wv / g / dwv is null", who);
  MAE_REQUIRE(ap_aligned16(dp) && ap_aligned16(ybar) && ap_aligned16(rstd) && ap_aligned16(wv) && ap_aligned16(g) && ap_aligned16(dwv) &&
              ap_aligned16(scratch), "%s: every buffer must be 16-byte aligned", who);
  const int64_t need = attn_probe_project_bwd_scratch_bytes(B, D, H);
  MAE_REQUIRE(scratch && scratch_bytes >= need, "%s: scratch_bytes = %lld, mae_attn_probe_project_bwd_scratch_bytes asks for %lld", who,
              (long long)scratch_bytes, (long long)need);
  const int D4 = D / 4, slices = ap_wv_slices(B), per_slice = (int)cdiv(B, slices);
  hipLaunchKernelGGL(ap_project_dgrad_kernel, dim3((unsigned)cdiv(cdiv(B, AP_IMG_TILE) * H * D4, 256)), dim3(256), 0, s, dp, rstd, wv, (int)B, D, H, g);
  MAE_LAUNCH_CHECK();
  const unsigned cols = (unsigned)cdiv((int64_t)D * D4, 256);
  hipLaunchKernelGGL(ap_project_wgrad_kernel, dim3(cols, (unsigned)cdiv(B, per_slice)), dim3(256), 0, s, dp, ybar, (int)B, D, H, per_slice,
                     (float*)scratch);
  MAE_LAUNCH_CHECK();
  MAE_TRY(launch_sum_partials((const float*)scratch, (int)cdiv(B, per_slice), D * D, dwv, nullptr, D * D, s));
  hipLaunchKernelGGL(ap_scale_columns_kernel, dim3(cols), dim3(256), 0, s, dwv, rstd, D);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int mae_attn_pool_fwd(const float* x, const float* mean, const float* uq, int64_t batch, int64_t tokens, int32_t dim, int32_t heads,
                                 float* ybar, float* lse, void* stream) {
  return mae::launch_attn_pool_fwd(x, mean, uq, batch, tokens, dim, heads, ybar, lse, (hipStream_t)stream);
}

extern "C" int64_t mae_attn_pool_bwd_scratch_bytes(int64_t batch, int64_t tokens, int32_t dim, int32_t heads) {
  return mae::attn_pool_bwd_scratch_bytes(batch, tokens, dim, heads);
}

extern "C" int mae_attn_pool_bwd(const float* x, const float* mean, const float* uq, const float* lse, const float* ybar, const float* g,
                                 int64_t batch, int64_t tokens, int32_t dim, int32_t heads, float* duq, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  return mae::launch_attn_pool_bwd(x, mean, uq, lse, ybar, g, batch, tokens, dim, heads, duq, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int mae_attn_probe_fold(const float* q, const float* wk, const float* rstd, int32_t dim, int32_t heads, float* uq, void* stream) {
  return mae::launch_attn_probe_fold(q, wk, rstd, dim, heads, uq, (hipStream_t)stream);
}

extern "C" int mae_attn_probe_fold_bwd(const float* duq, const float* q, const float* wk, const float* rstd, int32_t dim, int32_t heads, float* dq,
                                       float* dwk, void* stream) {
  return mae::launch_attn_probe_fold_bwd(duq, q, wk, rstd, dim, heads, dq, dwk, (hipStream_t)stream);
}

extern "C" int mae_attn_probe_project(const float* ybar, const float* rstd, const float* wv, int64_t batch, int32_t dim, int32_t heads, float* p,
                                      void* stream) {
  return mae::launch_attn_probe_project(ybar, rstd, wv, batch, dim, heads, p, (hipStream_t)stream);
}

extern "C" int64_t mae_attn_probe_project_bwd_scratch_bytes(int64_t batch, int32_t dim, int32_t heads) {
  return mae::attn_probe_project_bwd_scratch_bytes(batch, dim, heads);
}

extern "C" int mae_attn_probe_project_bwd(const float* dp, const float* ybar, const float* rstd, const float* wv, int64_t batch, int32_t dim,
                                          int32_t heads, float* g, float* dwv, void* scratch, int64_t scratch_bytes, void* stream) {
  return mae::launch_attn_probe_project_bwd(dp, ybar, rstd, wv, batch, dim, heads, g, dwv, scratch, scratch_bytes, (hipStream_t)stream);
}
