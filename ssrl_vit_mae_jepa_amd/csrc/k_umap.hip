// UMAP of n <= 16384 feature rows in the plane: exact neighbours with umap-learn's smooth distances and memberships,
// and the synchronous layout epoch.  Everything is fp32, every sum has an order fixed by the shapes alone, there are no atomics, nothing
// synchronises with the host, and every buffer is the caller's.  This object is compiled with -ffp-contract=off (Makefile): a product
// followed by a sum is two roundings unless it is written as fmaf, so `next` and the active set can be restated in numpy fp32 bit for bit.
//
// mae_umap_fuzzy_knn, three launches, the squared distances in an (n, round_up(n, 4)) scratch:
//   tsne_sqdist_kernel   (sqdist_dev.cuh) d2_ij = sum_c (x_ic - x_jc)^2, one fmaf per column in column order; symmetric bit for bit.
//   umap_row_kernel      one workgroup per row.  d_j = sqrtf(d2_j) (correctly rounded) stays in LDS (n floats <= 64 KiB).  k selection
//                        rounds: thread t takes the minimum of the 64-bit keys (bits of d_j << 32 | j) over j = t, t + 256, ..., then the
//                        xor butterfly, then the four waves; the winner's owner overwrites it with +inf.  d >= +0, so the key order is
//                        (distance, index) ascending.  Wave 0 then holds entry r in lane r: rho = the first entry > 0 (0 if none), and
//                        umap-learn's smooth_knn_dist search for sigma: lo = 0, hi = inf, mid = 1; at most 64 steps;
//                        psum = sum_{r = 1 .. k - 1} (d_r - rho > 0 ? e^(-((d_r - rho) / mid)) : 1), a butterfly over the lanes, so every
//                        lane holds the same bits and takes the same branch; stop when |psum - log2 k| < 1e-5; psum above: hi = mid,
//                        mid = (lo + hi) / 2; else lo = mid and mid doubles while hi = inf, else bisects.  With rho > 0 the row's floor
//                        sigma >= 1e-3 mean(d_0 .. d_{k-1}) is applied here; the row's sum goes to scratch for the global floor.
//   umap_memb_kernel     every workgroup adds the n row sums in the same fixed order (thread t: t, t + 256, ...; butterfly; waves in
//                        order); rows with rho = 0 get sigma >= 1e-3 sum / (n k); one thread per entry then writes
//                        memb = 0 for the point itself, 1 if d - rho <= 0 or sigma = 0, else e^(-((d - rho) / sigma)).
//
// mae_umap_epoch: one launch.  A wave owns row i of the CSR graph; a trip covers E = floor(64 / (rate + 1)) consecutive edges, lane l
// taking edge l / (rate + 1) of the trip in role s = l mod (rate + 1): s = 0 the attraction to col[e], s >= 1 negative sample s - 1.  The
// edge's lane 0 reads next[e] and broadcasts it; the edge fires iff next[e] <= t.  Negative sample s' of edge e (the global index, that
// is row_ptr[i] + position) in epoch t is point
//       k = (uint64(h) * n) >> 32,   h = mix(mix(seed, t), 16 e + s'),   mix(s, i) = fmix32(fmix32(i + 0x9E3779B9) ^ s)   (common.cuh)
// in uint32 arithmetic: 16 e + s' < 2^25 for the 2 n k <= 2^21 edges of the largest graph, so nothing wraps but the generator's own
// products.  Per (edge, role), with dx = y_i - y_o, d2 = fma(dx.x, dx.x, dx.y dx.y), pb = exp2f(b log2f(d2)), den = fma(a, pb, 1):
//       attraction  2 clip(c dx), c = ((-2 (a b)) (pb / d2)) / den;      repulsion  clip(c dx), c = (2 (gamma b)) / ((0.001f + d2) den)
// clip per coordinate to [-4, 4]; the term is 0 when d2 = 0, and for a negative sample when k = i.  A lane adds its trips' terms in
// order, then the xor butterfly: the order depends on the row's degree and the rate alone.  y_out[i] = fma(alpha, sum, y_in[i]); lane 0 of
// a firing edge writes next[e] + eps[e] (one fp32 add).  y_in is read only; rows of any degree (0, 1, thousands) take the one path.
#include "sqdist_dev.cuh"

namespace mae {

constexpr int UM_MIN_N = 8, UM_MAX_N = 16384, UM_MAX_DIM = 8192, UM_MIN_K = 2, UM_MAX_K = 64, UM_MAX_RATE = 16;
constexpr int UM_THREADS = 256;
constexpr int UM_SEARCH_STEPS = 64;
constexpr float UM_TOL = 1e-5f, UM_FLOOR = 1e-3f;
constexpr int UM_ROW_LDS_TAIL = 4 * 8 + UM_MAX_K * 4 * 2;   // the waves' keys, then the selected distances and indices

static bool umap_n_ok(int n) { return n >= UM_MIN_N && n <= UM_MAX_N; }
static int64_t umap_pitch(int n) { return round_up(n, 4); }
// the squared distances (n, pitch), the rows' sums (pitch), the rows' sigma before the global floor (pitch)
int64_t umap_scratch_bytes(int n, int dim, int k) {
  if (!umap_n_ok(n) || dim < 1 || dim > UM_MAX_DIM || k < UM_MIN_K || k > UM_MAX_K || k >= n) return -1;
  return (umap_pitch(n) * n + 2 * umap_pitch(n)) * (int64_t)sizeof(float);
}

// ---- neighbours, rho, sigma ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long um_min_key(unsigned long long a, unsigned long long b) { return a < b ? a : b; }

// LDS: d[pitch], keys of the four waves, sel_d[64], sel_i[64]
__global__ void __launch_bounds__(UM_THREADS) umap_row_kernel(const float* __restrict__ D, int pitch, int n, int k, float target,
                                                              int32_t* __restrict__ knn_idx, float* __restrict__ knn_dist, float* __restrict__ rho_out,
                                                              float* __restrict__ sigma_row, float* __restrict__ row_sum) {
  extern __shared__ __attribute__((aligned(16))) float um_lds[];
  float* d = um_lds;
  unsigned long long* red = reinterpret_cast<unsigned long long*>(um_lds + pitch);
  float* sel_d = reinterpret_cast<float*>(red + 4);
  int* sel_i = reinterpret_cast<int*>(sel_d + UM_MAX_K);
  const int t = threadIdx.x, i = blockIdx.x;
  const float* row = D + (int64_t)i * pitch;
  for (int j = t; j < n; j += UM_THREADS) d[j] = sqrtf(row[j]);   // a thread reads back only what it wrote
  for (int r = 0; r < k; ++r) {
    unsigned long long best = ~0ull;
    for (int j = t; j < n; j += UM_THREADS) best = um_min_key(best, ((unsigned long long)__float_as_uint(d[j]) << 32) | (unsigned)j);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned hi = __shfl_xor((unsigned)(best >> 32), o, 64), lo = __shfl_xor((unsigned)best, o, 64);
      best = um_min_key(best, ((unsigned long long)hi << 32) | lo);
    }
    if ((t & 63) == 0) red[t >> 6] = best;
    __syncthreads();
    best = um_min_key(um_min_key(red[0], red[1]), um_min_key(red[2], red[3]));
    const int jw = (int)(unsigned)best;   // < n: n >= 8 entries carry their own index, taken ones (+inf) included
    if ((jw & (UM_THREADS - 1)) == t) d[jw] = INFINITY;   // the owner takes it out
    if (t == 0) {
      sel_d[r] = __uint_as_float((unsigned)(best >> 32));
      sel_i[r] = jw;
    }
    __syncthreads();   // red is rewritten in the next round
  }
  if (t >= 64) return;   // wave 0: entry r in lane r
  const bool mine = t < k;
  const float dl = mine ? sel_d[t] : 0.f;
  const unsigned long long nz = __ballot(mine && dl > 0.f);
  const float rho = nz ? sel_d[__builtin_ctzll(nz)] : 0.f;
  const bool in_sum = mine && t >= 1;
  const float dr = dl - rho;
  float lo = 0.f, hi = INFINITY, mid = 1.f;
  for (int step = 0; step < UM_SEARCH_STEPS; ++step) {
    const float term = in_sum ? (dr > 0.f ? __expf(-(dr / mid)) : 1.f) : 0.f;
    const float psum = wave_sum(term);
    if (fabsf(psum - target) < UM_TOL) break;   // uniform: every lane holds the same sum
    if (psum > target) {
      hi = mid;
      mid = (lo + hi) * 0.5f;
    } else {
      lo = mid;
      mid = hi == INFINITY ? mid * 2.f : (lo + hi) * 0.5f;
    }
  }
  const float sum = wave_sum(dl);
  if (rho > 0.f) mid = fmaxf(mid, UM_FLOOR * (sum / (float)k));
  if (mine) {
    knn_idx[(int64_t)i * k + t] = sel_i[t];
    knn_dist[(int64_t)i * k + t] = dl;
  }
  if (t == 0) {
    rho_out[i] = rho;
    sigma_row[i] = mid;
    row_sum[i] = sum;
  }
}

__global__ void __launch_bounds__(UM_THREADS) umap_memb_kernel(const int32_t* __restrict__ knn_idx, const float* __restrict__ knn_dist,
                                                               const float* __restrict__ rho, const float* __restrict__ sigma_row,
                                                               const float* __restrict__ row_sum, int n, int k, float* __restrict__ sigma,
                                                               float* __restrict__ memb) {
  __shared__ float red[4];
  float s = 0.f;
  for (int j = threadIdx.x; j < n; j += UM_THREADS) s += row_sum[j];
  const float floor_all = UM_FLOOR * (block_sum_256(s, red) / (float)(n * k));   // the same bits in every workgroup
  const int e = blockIdx.x * UM_THREADS + threadIdx.x;
  if (e >= n * k) return;
  const int i = e / k;
  const float r = rho[i];
  float sg = sigma_row[i];
  if (!(r > 0.f)) sg = fmaxf(sg, floor_all);
  if (e == i * k) sigma[i] = sg;
  const float dd = knn_dist[e] - r;
  memb[e] = knn_idx[e] == i ? 0.f : (dd <= 0.f || sg == 0.f) ? 1.f : __expf(-(dd / sg));
}

int launch_umap_fuzzy_knn(const float* x, int n, int dim, int k, int32_t* knn_idx, float* knn_dist, float* memb, float* rho, float* sigma, void* scratch,
                          int64_t scratch_bytes, hipStream_t s) {
  const char* who = "umap_fuzzy_knn";
  MAE_REQUIRE(umap_n_ok(n), "%s: n = %d outside [%d, %d]", who, n, UM_MIN_N, UM_MAX_N);
  MAE_REQUIRE(dim >= 1 && dim <= UM_MAX_DIM, "%s: dim = %d outside [1, %d]", who, dim, UM_MAX_DIM);
  MAE_REQUIRE(k >= UM_MIN_K && k <= UM_MAX_K && k < n, "%s: n_neighbors = %d outside [%d, min(%d, n - 1 = %d)]", who, k, UM_MIN_K, UM_MAX_K, n - 1);
  MAE_REQUIRE(x && knn_idx && knn_dist && memb && rho && sigma && scratch, "%s: null x / knn_idx / knn_dist / memb / rho / sigma / scratch", who);
  MAE_REQUIRE((((uintptr_t)x | (uintptr_t)knn_idx | (uintptr_t)knn_dist | (uintptr_t)memb | (uintptr_t)rho | (uintptr_t)sigma) & 3) == 0 &&
                  ((uintptr_t)scratch & 15) == 0,
              "%s: scratch must be 16-byte aligned, every other buffer 4-byte", who);
  const int64_t need = umap_scratch_bytes(n, dim, k);
  MAE_REQUIRE(scratch_bytes >= need, "%s: scratch_bytes = %lld below mae_umap_scratch_bytes = %lld", who, (long long)scratch_bytes, (long long)need);
  const int pitch = (int)umap_pitch(n), nb = (int)cdiv(n, TS_TILE);
  float* D = (float*)scratch;
  float* row_sum = D + (int64_t)pitch * n;
  float* sigma_row = row_sum + pitch;
  hipLaunchKernelGGL(tsne_sqdist_kernel, dim3(nb, nb), dim3(TS_THREADS), 0, s, x, n, dim, D, pitch, (float*)nullptr);
  MAE_LAUNCH_CHECK();
  const size_t lds = (size_t)pitch * sizeof(float) + UM_ROW_LDS_TAIL;
  MAE_TRY(allow_lds(umap_row_kernel, lds));
  hipLaunchKernelGGL(umap_row_kernel, dim3(n), dim3(UM_THREADS), lds, s, (const float*)D, pitch, n, k, (float)log2((double)k), knn_idx, knn_dist, rho,
                     sigma_row, row_sum);
  MAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(umap_memb_kernel, dim3((unsigned)cdiv((int64_t)n * k, UM_THREADS)), dim3(UM_THREADS), 0, s, (const int32_t*)knn_idx,
                     (const float*)knn_dist, (const float*)rho, (const float*)sigma_row, (const float*)row_sum, n, k, sigma, memb);
  MAE_LAUNCH_CHECK();
  return 0;
}

// ---- the layout epoch ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float um_clip(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

__global__ void __launch_bounds__(UM_THREADS) umap_epoch_kernel(const float* __restrict__ y_in, float* __restrict__ y_out, const int32_t* __restrict__ row_ptr,
                                                                const int32_t* __restrict__ col, const float* __restrict__ eps, float* __restrict__ next, int n,
                                                                float a, float b, float gamma, float alpha, int t, int rate, uint32_t seed) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int i = blockIdx.x * (UM_THREADS / 64) + wv;
  if (i >= n) return;   // the wave's own row: no barrier follows
  const int e0 = row_ptr[i], e1 = row_ptr[i + 1];
  const float2 yi = reinterpret_cast<const float2*>(y_in)[i];
  const int per = rate + 1, trip = 64 / per;   // roles of an edge, edges of a trip
  const int le = lane / per, role = lane - le * per;
  const bool on = le < trip;
  const int head = on ? le * per : 0;          // the lane that reads the edge
  const float m2ab = -2.f * (a * b), c2gb = 2.f * (gamma * b), tf = (float)t;
  const uint32_t epoch_key = aug_mix(seed, (uint32_t)t);
  float sx = 0.f, sy = 0.f;
  for (int eb = e0; eb < e1; eb += trip) {   // uniform over the wave
    const int e = eb + le;
    const bool live = on && e < e1;
    float nx = INFINITY;
    if (live && role == 0) nx = next[e];
    nx = __shfl(nx, head, 64);
    if (!(live && nx <= tf)) continue;   // no shuffle follows in this trip
    int j;
    if (role == 0) {
      j = (int)min((unsigned)col[e], (unsigned)(n - 1));   // a column is never trusted as an index
      next[e] = nx + eps[e];
    } else {
      j = (int)__umulhi(aug_mix(epoch_key, 16u * (uint32_t)e + (uint32_t)(role - 1)), (uint32_t)n);
    }
    const float2 yo = reinterpret_cast<const float2*>(y_in)[j];
    const float dx = yi.x - yo.x, dy = yi.y - yo.y;
    const float d2 = fmaf(dx, dx, dy * dy);
    if (!(d2 > 0.f) || (role != 0 && j == i)) continue;
    const float pb = exp2f(b * log2f(d2));
    const float den = fmaf(a, pb, 1.f);
    if (role == 0) {
      const float c = (m2ab * (pb / d2)) / den;
      sx += 2.f * um_clip(c * dx);
      sy += 2.f * um_clip(c * dy);
    } else {
      const float c = c2gb / ((0.001f + d2) * den);
      sx += um_clip(c * dx);
      sy += um_clip(c * dy);
    }
  }
  sx = wave_sum(sx);
  sy = wave_sum(sy);
  if (lane == 0) reinterpret_cast<float2*>(y_out)[i] = make_float2(fmaf(alpha, sx, yi.x), fmaf(alpha, sy, yi.y));
}

int launch_umap_epoch(const float* y_in, float* y_out, const int32_t* row_ptr, const int32_t* col, const float* eps, float* next, int n, float a, float b,
                      float gamma, float alpha, int t, int rate, uint32_t seed, hipStream_t s) {
  const char* who = "umap_epoch";
  MAE_REQUIRE(umap_n_ok(n), "%s: n = %d outside [%d, %d]", who, n, UM_MIN_N, UM_MAX_N);
  MAE_REQUIRE(rate >= 1 && rate <= UM_MAX_RATE, "%s: negative_sample_rate = %d outside [1, %d]", who, rate, UM_MAX_RATE);
  MAE_REQUIRE(t >= 0 && t < (1 << 24), "%s: epoch t = %d outside [0, 2^24)", who, t);
  MAE_REQUIRE(a > 0.f && b > 0.f && a < INFINITY && b < INFINITY, "%s: curve (a, b) = (%g, %g) must be positive and finite", who, (double)a, (double)b);
  MAE_REQUIRE(y_in && y_out && row_ptr, "%s: null y_in / y_out / row_ptr", who);
  MAE_REQUIRE(y_in != y_out, "%s: y_out must not be y_in (the epoch is synchronous)", who);
  MAE_REQUIRE((((uintptr_t)y_in | (uintptr_t)y_out) & 15) == 0 && (((uintptr_t)row_ptr | (uintptr_t)col | (uintptr_t)eps | (uintptr_t)next) & 3) == 0,
              "%s: y_in and y_out must be 16-byte aligned, every other buffer 4-byte", who);
  hipLaunchKernelGGL(umap_epoch_kernel, dim3((unsigned)cdiv(n, UM_THREADS / 64)), dim3(UM_THREADS), 0, s, y_in, y_out, row_ptr, col, eps, next, n, a, b,
                     gamma, alpha, t, rate, seed);
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int64_t mae_umap_scratch_bytes(int32_t n, int32_t dim, int32_t n_neighbors) { return mae::umap_scratch_bytes(n, dim, n_neighbors); }
extern "C" int mae_umap_fuzzy_knn(const float* x, int32_t n, int32_t dim, int32_t n_neighbors, int32_t* knn_idx, float* knn_dist, float* memb, float* rho,
                                  float* sigma, void* scratch, int64_t scratch_bytes, void* stream) {
  return mae::launch_umap_fuzzy_knn(x, n, dim, n_neighbors, knn_idx, knn_dist, memb, rho, sigma, scratch, scratch_bytes, (hipStream_t)stream);
}
extern "C" int mae_umap_epoch(const float* y_in, float* y_out, const int32_t* row_ptr, const int32_t* col, const float* eps, float* next, int32_t n, float a,
                              float b, float gamma, float alpha, int32_t t, int32_t rate, uint32_t seed, void* stream) {
  return mae::launch_umap_epoch(y_in, y_out, row_ptr, col, eps, next, n, a, b, gamma, alpha, t, rate, seed, (hipStream_t)stream);
}
