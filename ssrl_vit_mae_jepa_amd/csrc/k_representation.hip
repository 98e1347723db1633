// Representation evaluation: pooled frozen-encoder features and the weighted k-NN probe on them.
// Reference: scripts/evaluation/visualize_representation.py:87-150 (forward_features -> pool -> optional normalisation);
// the k-NN probe has no reference code (DINO's weighted k-NN: cosine similarity, k = 20, T = 0.07; spec in DESIGN.md 11).
//
// (1) features_kernel: the residual add after any encoder block, the encoder's final LayerNorm in fp32, the pool and the optional
//     L2 step, one block per image, writing fp32 only: (B, D), or one slice of a (B, taps, W) buffer, where the pool
//     [class row | patch mean] has W = 2 D.
// (2) knn_search_kernel: fused similarity + per-query running top-k.  Query tiles of 32 x bank splits; each chunk of 128
//     bank rows is one 32x32 tile per wave on the fp32-input MFMA (exact fp32, a fixed fmaf order per pair, so the value
//     of a pair depends on the two rows alone), staged in LDS, then merged into the running lists behind a threshold test.
//     The (Q, splits, k) partial lists are merged by knn_merge_kernel.  Q x N is never written to memory.
// (3) knn_vote_kernel: scores[q][c] = sum_j [label(idx_j) == c] exp(sim_j / T) in j order, pred = argmax (lowest class).
// Order of every list: similarity descending, then bank index ascending; a NaN similarity is reported (and sorted) as -inf.
#include "kernels.h"

namespace mae {

// ---------------------------------------------------------------------------------------------------
// (1) add + LayerNorm + pool + L2 of the residual stream after an encoder block, into out + b * out_stride: (B, D), or one
// slice of a (B, taps, W) buffer; the pool [class row | patch mean] (W = 2 D) comes from one pass over the rows.
// ---------------------------------------------------------------------------------------------------
// The roundings are fixed in the text, because under -ffp-contract=fast the build would pick which a * b + c to fuse from the code
// around it (and pragmas or *_rn intrinsics do not stop it).  Fused (fmaf): LayerNorm's scale and shift, and the L2 sum
// fma(f0, f0, f1 * f1) + fma(f2, f2, f3 * f3).  Not fused (unfused_mul): the row's squares (d * d), and the inner products of the L2 sum.
__device__ __forceinline__ float unfused_mul(float a, float b) {
  float p = a * b;
  asm("" : "+v"(p));  // emits nothing; the product is opaque to the contraction of the addition that follows
  return p;
}
__device__ __forceinline__ float l2_sumsq4(f32x4 f) {  // the L2 term of one thread
  return __builtin_fmaf(f[0], f[0], unfused_mul(f[1], f[1])) + __builtin_fmaf(f[2], f[2], unfused_mul(f[3], f[3]));
}

// One row: a wave normalises it (lane owns columns 4 * (lane + 64 i)) and adds it to the wave's running sum.
template <class T>
__device__ __forceinline__ void features_add_row(const float* __restrict__ x_mid, const T* __restrict__ branch, const float* __restrict__ gamma,
                                                 const float* __restrict__ beta, float eps, int64_t r, int D, int D4, int lane, f32x4 (&acc)[4]) {
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 v[4];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < D4 ? load4(x_mid + r + 4 * c) + load4(branch + r + 4 * c) : z;
    s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
  }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (lane + 64 * i < D4) {
      const f32x4 d = v[i] - mean;
      q += (unfused_mul(d[0], d[0]) + unfused_mul(d[1], d[1])) + (unfused_mul(d[2], d[2]) + unfused_mul(d[3], d[3]));
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) {
      const f32x4 d = (v[i] - mean) * rstd, g = load4(gamma + 4 * c), h = load4(beta + 4 * c);
      const f32x4 y = {__builtin_fmaf(d[0], g[0], h[0]), __builtin_fmaf(d[1], g[1], h[1]), __builtin_fmaf(d[2], g[2], h[2]), __builtin_fmaf(d[3], g[3], h[3])};
      acc[i] += y;
    }
  }
}

// Rows [row_lo, row_hi) of the image are pooled: wave w takes rows row_lo + w, row_lo + w + 4, ... into its own running sum, and the
// four wave sums are added in wave order.  Fixed order everywhere, no atomics.  cls_row (MAE_POOL_CLS_MEAN_PATCHES, row_lo = 1): wave 0
// also takes row 0 into an accumulator of its own; the row goes to out[0, D), the patch mean to out[D, 2D), each L2-normalised on its
// own.  A lone row needs no wave sum and no division: with the accumulator started at +0, acc + 0 + 0 + 0 and acc / 1 return acc's
// bits, so out[0, D) is what MAE_POOL_CLS gives.
template <class T>
__global__ void __launch_bounds__(256) features_kernel(const float* __restrict__ x_mid, const T* __restrict__ branch,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       int seq, int D, int row_lo, int row_hi, int cls_row, int normalize,
                                                       float* __restrict__ out, int64_t out_stride) {
  __shared__ __attribute__((aligned(16))) float part[4][1024];
  __shared__ __attribute__((aligned(16))) float part_cls[1024];
  __shared__ float red[4];
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D4 = D / 4;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc[4] = {z, z, z, z};
  if (cls_row && wave == 0) {
    f32x4 acc_cls[4] = {z, z, z, z};
    features_add_row(x_mid, branch, gamma, beta, eps, (int64_t)b * seq * D, D, D4, lane, acc_cls);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = lane + 64 * i;
      if (c < D4) *reinterpret_cast<f32x4*>(&part_cls[4 * c]) = acc_cls[i];
    }
  }
  for (int j = row_lo + wave; j < row_hi; j += 4) features_add_row(x_mid, branch, gamma, beta, eps, ((int64_t)b * seq + j) * D, D, D4, lane, acc);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = lane + 64 * i;
    if (c < D4) *reinterpret_cast<f32x4*>(&part[wave][4 * c]) = acc[i];
  }
  __syncthreads();
  f32x4 f = z;
  if (t < D4) {
    f = *reinterpret_cast<const f32x4*>(&part[0][4 * t]);
    for (int w = 1; w < 4; ++w) f += *reinterpret_cast<const f32x4*>(&part[w][4 * t]);
    f = f / (float)(row_hi - row_lo);
  }
  if (normalize == MAE_FEAT_L2) {  // f / (||f||_2 + 1e-8)
    const float ss = block_sum_256(l2_sumsq4(f), red);
    f = f / (sqrtf(ss) + 1e-8f);
  }
  float* o = out + (int64_t)b * out_stride;
  if (t < D4) store4(o + (cls_row ? D : 0) + 4 * t, f);
  if (!cls_row) return;
  f32x4 g = z;
  if (t < D4) g = *reinterpret_cast<const f32x4*>(&part_cls[4 * t]);
  if (normalize == MAE_FEAT_L2) {  // block_sum_256 opens with a barrier: every read of red above is over before it is rewritten
    const float ss = block_sum_256(l2_sumsq4(g), red);
    g = g / (sqrtf(ss) + 1e-8f);
  }
  if (t < D4) store4(o + 4 * t, g);
}

int features_tap_width(int pool, int D) { return pool == MAE_POOL_CLS_MEAN_PATCHES ? 2 * D : D; }

// The one launch of features_kernel and the rules every caller shares; `who` names the C entry in the messages.
static int launch_features(const char* who, const float* x_mid, const void* branch, int branch_dt, const float* gamma, const float* beta,
                           float eps, int B, int seq, int D, int row_lo, int row_hi, int cls_row, int normalize, float* out,
                           int64_t out_stride, hipStream_t s) {
  MAE_REQUIRE(x_mid && branch && gamma && beta && out, "%s: null argument", who);
  MAE_REQUIRE(B > 0 && seq > 0, "%s: batch = %d and seq_len = %d must be positive", who, B, seq);
  MAE_REQUIRE(D % 4 == 0 && D >= 4 && D <= 1024, "%s: dim = %d must be a multiple of 4 in [4, 1024]", who, D);
  MAE_REQUIRE(branch_dt == MAE_F32 || branch_dt == MAE_BF16, "%s: branch_dtype = %d, but the branch dtype must be MAE_F32 or MAE_BF16", who, branch_dt);
  MAE_REQUIRE(normalize == MAE_FEAT_NONE || normalize == MAE_FEAT_L2, "%s: normalize must be MAE_FEAT_NONE or MAE_FEAT_L2 (got %d)", who, normalize);
  MAE_REQUIRE(row_lo >= 0 && row_lo < row_hi && row_hi <= seq, "%s: rows [%d, %d) outside the sequence of %d", who, row_lo, row_hi, seq);
  if (branch_dt == MAE_BF16)
    hipLaunchKernelGGL(features_kernel<bf16>, dim3(B), dim3(256), 0, s, x_mid, (const bf16*)branch, gamma, beta, eps, seq, D, row_lo, row_hi, cls_row,
                       normalize, out, out_stride);
  else
    hipLaunchKernelGGL(features_kernel<float>, dim3(B), dim3(256), 0, s, x_mid, (const float*)branch, gamma, beta, eps, seq, D, row_lo, row_hi, cls_row,
                       normalize, out, out_stride);
  MAE_LAUNCH_CHECK();
  return 0;
}

int launch_features_tap(const float* x_mid, const void* branch, int branch_dt, const float* gamma, const float* beta, float eps, int B, int seq,
                        int D, int with_cls, int pool, int normalize, float* out, int64_t out_stride, hipStream_t s) {
  const char* who = "mae_features_tap";
  const bool both = pool == MAE_POOL_CLS_MEAN_PATCHES;
  if (both) MAE_REQUIRE(with_cls == 1, "%s: pool MAE_POOL_CLS_MEAN_PATCHES needs with_cls = 1 (got %d)", who, with_cls);
  else MAE_TRY(check_pool(with_cls, pool, true, who));
  const int lo = (both || pool == MAE_POOL_MEAN_PATCHES) && with_cls ? 1 : 0, hi = pool == MAE_POOL_CLS ? 1 : seq;
  MAE_REQUIRE(seq <= 0 || lo < hi, "%s: seq_len = %d leaves no patch row behind the class row (pool %d needs seq_len >= 2)", who, seq, pool);
  const int W = features_tap_width(pool, D);
  MAE_REQUIRE(out_stride >= W && out_stride % 4 == 0, "%s: out_row_stride = %lld must be a multiple of 4 and at least the width %d", who,
              (long long)out_stride, W);
  return launch_features(who, x_mid, branch, branch_dt, gamma, beta, eps, B, seq, D, lo, hi, (int)both, normalize, out, out_stride, s);
}

// ---------------------------------------------------------------------------------------------------
// (2) top-k search
// ---------------------------------------------------------------------------------------------------
constexpr int KNN_QT = 32;            // queries per workgroup: the row tile of one 32x32 MFMA
constexpr int KNN_NT = 128;            // bank rows per chunk: one 32-column tile per wave
constexpr int KNN_SP = KNN_NT + 4;     // LDS pitch of the similarity tile
constexpr int KNN_MAX_K = 256;         // lane l of a wave owns list positions 4l .. 4l+3
constexpr int KNN_MERGE_MAX = 8192;    // candidates per query in the merge (splits * k), held in LDS
// Workgroups the splits aim for: 2 per CU of an MI355X where the LDS allows it (k <= 232; at k = 256 a workgroup holds
// 82,432 B of LDS and one fits per CU).  A constant, so results never depend on the device.
constexpr int KNN_TARGET_WGS = 512;
constexpr int KNN_SENTINEL = 0x7fffffff;  // index of an empty list slot: loses every tie against a real bank row

__device__ __forceinline__ bool knn_better(float va, int ia, float vb, int ib) { return va > vb || (va == vb && ia < ib); }

template <class V>
__device__ __forceinline__ V pick4(const V (&a)[4], int u) { return u == 0 ? a[0] : u == 1 ? a[1] : u == 2 ? a[2] : a[3]; }

int knn_splits(int64_t Q, int64_t N, int k) {
  const int64_t qt = cdiv(Q, KNN_QT);
  int64_t S = cdiv(KNN_TARGET_WGS, qt);
  S = std::min<int64_t>(S, cdiv(N, KNN_NT));
  S = std::min<int64_t>(S, KNN_MERGE_MAX / k);
  return (int)std::max<int64_t>(S, 1);
}

static int next_pow2(int n) {
  int m = 1;
  while (m < n) m <<= 1;
  return m;
}

__global__ void __launch_bounds__(256) knn_search_kernel(const float* __restrict__ Qm, int64_t Q, const float* __restrict__ Bm, int64_t N, int D,
                                                         int k, int KP, int S, float* __restrict__ part_v, int32_t* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* st = smem;                                    // [QT][SP] similarity tile
  float* lv = st + KNN_QT * KNN_SP;                    // [QT][KP] running lists: values
  int* li = reinterpret_cast<int*>(lv + KNN_QT * KP);  //                        bank indices
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.x * KNN_QT;
  const int sp = blockIdx.y;
  const int64_t n_lo = N * sp / S, n_hi = N * (sp + 1) / S;
  for (int i = t; i < KNN_QT * KP; i += 256) { lv[i] = -INFINITY; li[i] = KNN_SENTINEL; }
  // MFMA 32x32x2 f32 operands: lane (r, h) feeds A[r][k = h] and B[k = h][r].  Each lane loads 4 consecutive columns
  // 8j + 4h .. 8j + 4h + 3 of its row, so step u of chunk j multiplies columns 8j + u (k = 0) and 8j + 4 + u (k = 1):
  // every pair is the same fmaf chain in the same column order whatever the tile, the split or Q.
  const float* qp = Qm + std::min<int64_t>(q0 + r, Q - 1) * D + 4 * h;
  const int D8 = D / 8;
  const bool tail = (D & 4) != 0;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  for (int64_t cb = n_lo; cb < n_hi; cb += KNN_NT) {
    const float* bp = Bm + std::min<int64_t>(cb + 32 * wave + r, n_hi - 1) * D + 4 * h;  // columns past n_hi are masked below
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll 2
    for (int j = 0; j < D8; ++j) {
      const f32x4 a = load4(qp + 8 * j), bb = load4(bp + 8 * j);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bb[u], acc, 0, 0, 0);
    }
    if (tail) {  // D = 8 * D8 + 4: the last four columns ride on k = 0, k = 1 multiplies zeros
      f32x4 a = z, bb = z;
      if (h == 0) { a = load4(qp + 8 * D8); bb = load4(bp + 8 * D8); }
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], bb[u], acc, 0, 0, 0);
    }
    // C/D map of the 32x32 tile: register i of lane (r, h) is row (i & 3) + 8 (i >> 2) + 4 h, column r
#pragma unroll
    for (int i = 0; i < 16; ++i) st[((i & 3) + 8 * (i >> 2) + 4 * h) * KNN_SP + 32 * wave + r] = acc[i];
    __syncthreads();
    // running lists: wave w owns queries w, w + 4, ...; candidates that beat the k-th entry are inserted one at a time
    for (int qi = wave; qi < KNN_QT && q0 + qi < Q; qi += 4) {
      float ev[4];
      int ei[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = 4 * lane + u;
        ev[u] = p < KP ? lv[qi * KP + p] : -INFINITY;
        ei[u] = p < KP ? li[qi * KP + p] : KNN_SENTINEL;
      }
      float tv = __shfl(pick4(ev, (k - 1) & 3), (k - 1) >> 2);
      int ti = __shfl(pick4(ei, (k - 1) & 3), (k - 1) >> 2);
      for (int c0 = 0; c0 < KNN_NT; c0 += 64) {
        const int64_t n = cb + c0 + lane;
        float v = st[qi * KNN_SP + c0 + lane];
        v = v != v ? -INFINITY : v;  // NaN sorts as -inf
        uint64_t m = __ballot(n < n_hi && knn_better(v, (int)n, tv, ti));
        while (m) {
          const int src = __builtin_ctzll(m);
          m &= m - 1;
          const float cv = __shfl(v, src);
          const int ci = __shfl((int)n, src);
          if (!knn_better(cv, ci, tv, ti)) continue;  // the threshold rose since the ballot
          int pos = 0;  // entries ahead of the candidate (the list is sorted, so they form a prefix)
#pragma unroll
          for (int u = 0; u < 4; ++u) pos += __popcll(__ballot(4 * lane + u < k && knn_better(ev[u], ei[u], cv, ci)));
          const float pv = __shfl_up(ev[3], 1);
          const int pi = __shfl_up(ei[3], 1);
          float nv[4];
          int ni[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int p = 4 * lane + u;
            nv[u] = ev[u]; ni[u] = ei[u];
            if (p < k && p == pos) { nv[u] = cv; ni[u] = ci; }
            else if (p < k && p > pos) { nv[u] = u == 0 ? pv : ev[u - 1]; ni[u] = u == 0 ? pi : ei[u - 1]; }
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) { ev[u] = nv[u]; ei[u] = ni[u]; }
          tv = __shfl(pick4(ev, (k - 1) & 3), (k - 1) >> 2);
          ti = __shfl(pick4(ei, (k - 1) & 3), (k - 1) >> 2);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = 4 * lane + u;
        if (p < KP) { lv[qi * KP + p] = ev[u]; li[qi * KP + p] = ei[u]; }
      }
    }
    __syncthreads();
  }
  for (int i = t; i < KNN_QT * k; i += 256) {
    const int qi = i / k, p = i - qi * k;
    if (q0 + qi >= Q) break;
    const int64_t o = ((q0 + qi) * S + sp) * k + p;
    part_v[o] = lv[qi * KP + p];
    part_i[o] = li[qi * KP + p];
  }
}

// One block per query: bitonic sort of the query's S * k partial entries (padded to a power of two with empty slots),
// the first k leave.  The comparison is a total order on (value, index), so the result does not depend on the splits.
__global__ void __launch_bounds__(256) knn_merge_kernel(const float* __restrict__ part_v, const int32_t* __restrict__ part_i, int n, int M, int k,
                                                        float* __restrict__ out_v, int64_t* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) float msm[];
  float* mv = msm;
  int* mi = reinterpret_cast<int*>(msm + M);
  const int t = threadIdx.x;
  const int64_t q = blockIdx.x;
  for (int i = t; i < M; i += 256) {
    mv[i] = i < n ? part_v[q * n + i] : -INFINITY;
    mi[i] = i < n ? part_i[q * n + i] : KNN_SENTINEL;
  }
  __syncthreads();
  for (int size = 2; size <= M; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = t; i < M / 2; i += 256) {
        const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
        const float a = mv[lo], b = mv[hi];
        const int ia = mi[lo], ib = mi[hi];
        const bool first = (lo & size) == 0;  // this run ends better-first
        if (first ? knn_better(b, ib, a, ia) : knn_better(a, ia, b, ib)) { mv[lo] = b; mv[hi] = a; mi[lo] = ib; mi[hi] = ia; }
      }
      __syncthreads();
    }
  }
  for (int p = t; p < k; p += 256) {
    out_v[q * k + p] = mv[p];
    out_i[q * k + p] = mi[p];
  }
}

int64_t knn_scratch_bytes(int64_t Q, int64_t N, int D, int k) {
  if (Q < 1 || N < 1 || N >= (1ll << 31) || D < 4 || D > 4096 || D % 4 != 0 || k < 1 || k > KNN_MAX_K || k > N) return -1;
  const int64_t n = Q * knn_splits(Q, N, k) * k;
  return round_up(n * 4, 256) + round_up(n * 4, 256);
}

int launch_knn_topk(const float* queries, int64_t Q, const float* bank, int64_t N, int D, int k, float* topk_sim, int64_t* topk_idx,
                    void* scratch, int64_t scratch_bytes, hipStream_t s) {
  MAE_REQUIRE(queries && bank && topk_sim && topk_idx && scratch, "mae_knn_topk: null argument");
  MAE_REQUIRE(Q >= 1 && N >= 1 && N < (1ll << 31), "mae_knn_topk: num_queries = %lld, bank_size = %lld (need >= 1 and bank < 2^31)", (long long)Q, (long long)N);
  MAE_REQUIRE(D % 4 == 0 && D >= 4 && D <= 4096, "mae_knn_topk: dim = %d must be a multiple of 4 in [4, 4096]", D);
  MAE_REQUIRE(k >= 1 && k <= KNN_MAX_K && k <= N, "mae_knn_topk: k = %d outside [1, min(%d, bank_size = %lld)]", k, KNN_MAX_K, (long long)N);
  MAE_REQUIRE(((uintptr_t)queries & 15) == 0 && ((uintptr_t)bank & 15) == 0 && ((uintptr_t)scratch & 255) == 0,
              "mae_knn_topk: queries / bank must be 16-byte aligned, scratch 256-byte");
  const int64_t need = knn_scratch_bytes(Q, N, D, k);
  MAE_REQUIRE(scratch_bytes >= need, "mae_knn_topk: scratch too small (%lld < %lld bytes)", (long long)scratch_bytes, (long long)need);
  const int S = knn_splits(Q, N, k);
  const int KP = (int)round_up(k, 4);
  const int64_t n = Q * S * k;
  float* part_v = reinterpret_cast<float*>(scratch);
  int32_t* part_i = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(scratch) + round_up(n * 4, 256));
  const int lds = (KNN_QT * KNN_SP + 2 * KNN_QT * KP) * 4;
  MAE_HIP(hipFuncSetAttribute((const void*)knn_search_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipLaunchKernelGGL(knn_search_kernel, dim3((unsigned)cdiv(Q, KNN_QT), S), dim3(256), lds, s, queries, Q, bank, N, D, k, KP, S, part_v, part_i);
  MAE_LAUNCH_CHECK();
  const int M = next_pow2(S * k);
  hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)Q), dim3(256), M * 8, s, part_v, part_i, S * k, M, k, topk_sim, topk_idx);
  MAE_LAUNCH_CHECK();
  return 0;
}

// ---------------------------------------------------------------------------------------------------
// (3) weighted vote
// ---------------------------------------------------------------------------------------------------
// One block per query, thread c owns class c: it walks the first k neighbours in order and adds exp(sim / T) of those
// labelled c.  A label outside [0, C) is never used as an index: the query's scores become NaN and its prediction -1.
__global__ void __launch_bounds__(HEAD_MAX_CLASSES) knn_vote_kernel(const float* __restrict__ sim, const int64_t* __restrict__ idx, int k_stride,
                                                                    int k, const int64_t* __restrict__ labels, int C, float T,
                                                                    float* __restrict__ scores, int64_t* __restrict__ pred) {
  __shared__ float sc[HEAD_MAX_CLASSES];
  const int64_t q = blockIdx.x;
  const int c = threadIdx.x;
  float acc = 0.f;
  bool bad = false;
  for (int j = 0; j < k; ++j) {
    const int64_t i = idx[q * k_stride + j];
    const int64_t y = i >= 0 ? labels[i] : -1;
    if (y < 0 || y >= C) { bad = true; continue; }
    if (y == c) acc += expf(sim[q * k_stride + j] / T);
  }
  if (bad) acc = __builtin_nanf("");
  if (c < C) sc[c] = acc;
  __syncthreads();
  if (scores && c < C) scores[q * C + c] = acc;
  if (c == 0) {
    int best = 0;
    for (int j = 1; j < C; ++j)
      if (sc[j] > sc[best]) best = j;
    pred[q] = bad ? -1 : best;
  }
}

int launch_knn_vote(const float* sim, const int64_t* idx, int64_t Q, int k_stride, int k, const int64_t* labels, int C, float T, float* scores,
                    int64_t* pred, hipStream_t s) {
  MAE_REQUIRE(sim && idx && labels && pred, "mae_knn_vote: null argument");
  MAE_REQUIRE(Q >= 1 && Q < (1ll << 31), "mae_knn_vote: num_queries = %lld outside [1, 2^31)", (long long)Q);
  MAE_REQUIRE(k >= 1 && k <= k_stride, "mae_knn_vote: k = %d outside [1, k_stride = %d]", k, k_stride);
  MAE_REQUIRE(C >= 2 && C <= HEAD_MAX_CLASSES, "mae_knn_vote: num_classes = %d outside [2, %d]", C, HEAD_MAX_CLASSES);
  MAE_REQUIRE(T > 0.f && std::isfinite(T), "mae_knn_vote: temperature %g must be positive", (double)T);
  hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)Q), dim3(HEAD_MAX_CLASSES), 0, s, sim, idx, k_stride, k, labels, C, T, scores, pred);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

// single-kernel entries (parity tests): features_kernel on caller buffers, by row range or by (with_cls, pool); see mae_hip.h
extern "C" int mae_features_pool(const float* x_mid, const void* branch, int32_t branch_dtype, const float* gamma, const float* beta, float eps,
                                 int32_t batch, int32_t seq_len, int32_t dim, int32_t row_lo, int32_t row_hi, int32_t normalize, float* out,
                                 void* stream) {
  return mae::launch_features("mae_features_pool", x_mid, branch, branch_dtype, gamma, beta, eps, batch, seq_len, dim, row_lo, row_hi, 0, normalize, out,
                              dim, (hipStream_t)stream);
}

extern "C" int mae_features_tap(const float* x_mid, const void* branch, int32_t branch_dtype, const float* gamma, const float* beta, float eps,
                                int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t pool, int32_t normalize, float* out,
                                int64_t out_row_stride, void* stream) {
  MAE_REQUIRE(((uintptr_t)out & 15) == 0, "mae_features_tap: out must be 16-byte aligned");
  return mae::launch_features_tap(x_mid, branch, branch_dtype, gamma, beta, eps, batch, seq_len, dim, with_cls, pool, normalize, out,
                                  out_row_stride, (hipStream_t)stream);
}

extern "C" int64_t mae_knn_scratch_bytes(int64_t num_queries, int64_t bank_size, int32_t dim, int32_t k) {
  return mae::knn_scratch_bytes(num_queries, bank_size, dim, k);
}

extern "C" int mae_knn_topk(const float* queries, int64_t num_queries, const float* bank, int64_t bank_size, int32_t dim, int32_t k, float* topk_sim,
                            int64_t* topk_idx, void* scratch, int64_t scratch_bytes, void* stream) {
  return mae::launch_knn_topk(queries, num_queries, bank, bank_size, dim, k, topk_sim, topk_idx, scratch, scratch_bytes, (hipStream_t)stream);
}

extern "C" int mae_knn_vote(const float* topk_sim, const int64_t* topk_idx, int64_t num_queries, int32_t k_stride, int32_t k, const int64_t* bank_labels,
                            int32_t num_classes, float temperature, float* scores, int64_t* pred, void* stream) {
  return mae::launch_knn_vote(topk_sim, topk_idx, num_queries, k_stride, k, bank_labels, num_classes, temperature, scores, pred, (hipStream_t)stream);
}
