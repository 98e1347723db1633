// The linear-probe sweep: G heads on the same BatchNorm output in one pass, and the LARS step of G segments in one call.
// BatchNorm1d(affine=False) has no per-head state, so the G heads of a learning-rate / weight-decay grid are two GEMMs over
// n = (g, c), the stacked class index of NC = G C columns:
//   forward           logits[g][b][c] = sum_d y[b][d] W_g[c][d] + b_g[c]
//   weight gradient   dW_g[c][d] = sum_b dlogits[b][n] y[b][d],  db_g[c] = sum_b dlogits[b][n],  dlogits = (softmax - onehot) / rows
// Both run on the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain, bit for bit), as knn_search_kernel does.
//
// Every output element is one chain of its own whose order depends on (rows, dim) alone, never on G, on the head's position in the
// stack or on the tile it falls into, so head g's bits are those of the same head run alone.  No atomics anywhere.
//
// sweep_fwd_kernel.  A workgroup owns 32 rows x 128 stacked columns (wave w the 32-column tile w) and walks D in chunks of 32 columns
// staged through LDS: y's and W's rows are D floats apart, so the MFMA's one-lane-per-row operand map would touch a cache line per
// lane from global memory; the float4 staging loads are coalesced (8 lanes per 128-byte row piece) and the LDS image has a pitch of
// 36 floats.  Lane (r, h) of a wave feeds A[r][k = h] and B[k = h][r]; from the float4 at columns 8j + 4h of its row, step u
// multiplies columns 8j + u (k = 0) and 8j + 4 + u (k = 1): the column order of every chain is 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ...
// Columns past D are staged as zeros (D = 8q + 4: the last k = 1 operands), rows past the end repeat the last row and are not stored.
//
// sweep_softmax_kernel.  One wave per (row, head) over the logits: lane l holds classes l and l + 64.
//
// sweep_wgrad_kernel.  A[i = n][k = b] = dlogits[b][n] and B[k = b][j = d] = y[b][d] are contiguous along the lanes' i and j index,
// so both operands come straight from global memory, one dword per lane and 128 bytes per half-wave, without LDS.  A wave owns
// 32 stacked classes x 128 feature columns (4 accumulator tiles: 5 loads per 4 MFMAs); the 4 waves of a workgroup take 4 class
// tiles of the same columns.  The batch is cut into S = sweep_slices(rows) slices [rows s / S, rows (s + 1) / S) on blockIdx.z; a step
// multiplies rows b (k = 0) and b + 1 (k = 1), a row past the slice's end enters as zeros.  The lanes of the column-tile-0
// workgroups also add their own dlogits operand: db = (sum over the even steps' rows) + (sum over the odd ones').  The partials
// (S, G, HF) are added in slice order by launch_sum_partials; each slice's padding is written as zeros.
#include "kernels.h"
#include "lars_dev.cuh"

namespace mae {

constexpr int SW_MAX_HEADS = 64;
constexpr int SW_FR = 32, SW_FC = 128, SW_FK = 32, SW_FP = SW_FK + 4;  // forward: rows, stacked columns, chunk and LDS pitch
constexpr int SW_WD = 128;                                              // weight gradient: feature columns per wave
constexpr int SW_SLICE_ROWS = 128, SW_MAX_SLICES = 16;

static bool sweep_rows_ok(int64_t rows, int C, int G) { return rows >= 1 && rows < ((int64_t)1 << 31) && rows * G * C < ((int64_t)1 << 31); }
static int sweep_slices(int64_t rows) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(rows, SW_SLICE_ROWS), SW_MAX_SLICES)); }
static int64_t sweep_hf(int C, int D) { return round_up((int64_t)C * D + C, 4); }

__global__ void __launch_bounds__(256) sweep_fwd_kernel(const float* __restrict__ y, int rows, int D, const float* __restrict__ heads, int C,
                                                        int NC, int64_t HF, float* __restrict__ logits) {
  __shared__ __attribute__((aligned(16))) float ys[SW_FR * SW_FP];
  __shared__ __attribute__((aligned(16))) float ws[SW_FC * SW_FP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int row0 = blockIdx.x * SW_FR, col0 = blockIdx.y * SW_FC;
  // staging: thread t loads the float4 at columns 4 (t & 7) of tile row t >> 3 (y) and of tile rows (t >> 3) + 32 p (W)
  const int sr = t >> 3, sc = 4 * (t & 7);
  const float* yp = y + (int64_t)min(row0 + sr, rows - 1) * D + sc;
  const float* wp[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int n = min(col0 + sr + 32 * p, NC - 1), g = n / C;
    wp[p] = heads + g * HF + (int64_t)(n - g * C) * D + sc;
  }
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int k0 = 0; k0 < D; k0 += SW_FK) {
    const bool in = k0 + sc < D;
    const f32x4 yv = in ? load4(yp + k0) : z;
    f32x4 wv[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) wv[p] = in ? load4(wp[p] + k0) : z;
    __syncthreads();  // the previous chunk has been read
    store4(&ys[sr * SW_FP + sc], yv);
#pragma unroll
    for (int p = 0; p < 4; ++p) store4(&ws[(sr + 32 * p) * SW_FP + sc], wv[p]);
    __syncthreads();
    const int steps = min(SW_FK, D - k0 + 4) / 8;  // 8-column steps that hold a column below D
#pragma unroll 4
    for (int j = 0; j < steps; ++j) {
      const f32x4 a = load4(&ys[r * SW_FP + 8 * j + 4 * h]), b = load4(&ws[(32 * wave + r) * SW_FP + 8 * j + 4 * h]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u], b[u], acc, 0, 0, 0);
    }
  }
  // C/D map of the 32x32 tile: register i of lane (r, h) is row (i & 3) + 8 (i >> 2) + 4 h, column r
  const int n = col0 + 32 * wave + r;
  if (n >= NC) return;
  const int g = n / C, c = n - g * C;
  const float bias = heads[g * HF + (int64_t)C * D + c];
  float* out = logits + (int64_t)g * rows * C + c;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int b = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (b < rows) out[(int64_t)b * C] = acc[i] + bias;
  }
}

// Wave (b, g): max-subtracted log-sum-exp, the first index among equal maxima (torch.argmax), the row's loss and correct flag and,
// when dlogits is given, dlogits[b][g C + c] = (softmax - onehot) / rows.  A label outside [0, C) is never used as an index: the
// row's loss and its dlogits are NaN and the row does not count as correct.
__global__ void __launch_bounds__(256) sweep_softmax_kernel(const float* __restrict__ logits, int rows, int C, int G,
                                                            const int64_t* __restrict__ labels, float* __restrict__ row_loss,
                                                            int32_t* __restrict__ row_correct, float* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= (int64_t)rows * G) return;
  const int g = (int)(w / rows), b = (int)(w - (int64_t)g * rows);
  const float* lp = logits + w * C;
  const bool in0 = lane < C, in1 = lane + 64 < C;
  const float l0 = in0 ? lp[lane] : -INFINITY, l1 = in1 ? lp[lane + 64] : -INFINITY;
  const float mx = wave_max(fmaxf(l0, l1));
  int am = l0 == mx ? lane : (l1 == mx ? lane + 64 : 0x7fffffff);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
  const float se = wave_sum((in0 ? expf(l0 - mx) : 0.f) + (in1 ? expf(l1 - mx) : 0.f));
  const float lse = mx + logf(se);
  const int64_t yl = labels[b];
  const bool valid = yl >= 0 && yl < C;
  const int yi = valid ? (int)yl : 0;
  const float v0 = __shfl(l0, yi & 63, 64), v1 = __shfl(l1, yi & 63, 64);
  if (lane == 0) {
    row_loss[w] = valid ? lse - (yi < 64 ? v0 : v1) : __builtin_nanf("");
    row_correct[w] = (valid && am == yi) ? 1 : 0;
  }
  if (!dlogits) return;
  float* dp = dlogits + (int64_t)b * G * C + (int64_t)g * C;
  const float nan = __builtin_nanf("");
  if (in0) dp[lane] = valid ? (expf(l0 - lse) - (lane == yi ? 1.f : 0.f)) / (float)rows : nan;
  if (in1) dp[lane + 64] = valid ? (expf(l1 - lse) - (lane + 64 == yi ? 1.f : 0.f)) / (float)rows : nan;
}

// block g: loss[g] = mean of the head's row losses, correct[g] = its count of correct rows; classifier_reduce_kernel's order
__global__ void __launch_bounds__(256) sweep_reduce_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ row_correct, int rows,
                                                           float* __restrict__ loss_out, int32_t* __restrict__ correct_out) {
  __shared__ float sl[256];
  __shared__ int sc[256];
  const int t = threadIdx.x, g = blockIdx.x;
  float l = 0.f;
  int n = 0;
  for (int b = t; b < rows; b += 256) { l += row_loss[(int64_t)g * rows + b]; n += row_correct[(int64_t)g * rows + b]; }
  sl[t] = l; sc[t] = n;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { sl[t] += sl[t + w]; sc[t] += sc[t + w]; }
    __syncthreads();
  }
  if (t == 0) {
    loss_out[g] = sl[0] / (float)rows;
    correct_out[g] = sc[0];
  }
}

__global__ void __launch_bounds__(256) sweep_wgrad_kernel(const float* __restrict__ dlogits, const float* __restrict__ y, int rows, int D, int C,
                                                          int NC, int64_t HF, int G, float* __restrict__ partial) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int S = gridDim.z, sl = blockIdx.z;
  const int b0 = (int)((int64_t)rows * sl / S), b1 = (int)((int64_t)rows * (sl + 1) / S);
  float* part = partial + (int64_t)sl * G * HF;
  if (blockIdx.x == 0 && blockIdx.y == 0) {  // the padding behind every head's db
    const int pad = (int)(HF - ((int64_t)C * D + C));
    for (int i = t; i < G * pad; i += 256) part[(i / pad) * HF + (int64_t)C * D + C + i % pad] = 0.f;
  }
  const int n0 = (blockIdx.x * 4 + wave) * 32, d0 = blockIdx.y * SW_WD;
  if (n0 >= NC) return;
  const int n = n0 + r;
  const float* ap = dlogits + min(n, NC - 1);  // a column past NC repeats the last one and is not stored
  const float* bp[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) bp[q] = y + min(d0 + 32 * q + r, D - 1);
  f32x16 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;
  float dbs = 0.f;
#pragma unroll 2
  for (int b = b0 + h; b < b1 + h; b += 2) {  // lane half h multiplies row b; both halves make the same number of steps
    const bool in = b < b1;
    const int br = in ? b : b1 - 1;
    float a = ap[(int64_t)br * NC], bv[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bv[q] = bp[q][(int64_t)br * D];
    if (!in) {
      a = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) bv[q] = 0.f;
    }
    dbs += a;
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv[q], acc[q], 0, 0, 0);
  }
  const float dbo = __shfl(dbs, r + 32, 64);  // the odd steps' rows
  if (blockIdx.y == 0 && h == 0 && n < NC) {
    const int g = n / C;
    part[g * HF + (int64_t)C * D + (n - g * C)] = dbs + dbo;
  }
  // register i of lane (r, h): row (class) (i & 3) + 8 (i >> 2) + 4 h, column (feature) r
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int nn = n0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (nn >= NC) continue;
    const int g = nn / C;
    float* out = part + g * HF + (int64_t)(nn - g * C) * D;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int d = d0 + 32 * q + r;
      if (d < D) out[d] = acc[q][i];
    }
  }
}

struct SweepScratch { float *logits, *dlogits, *row_loss; int32_t* row_correct; float* partial; int64_t floats; };
static SweepScratch sweep_scratch(void* scratch, int64_t rows, int D, int C, int G) {
  auto seg = [](int64_t n) { return round_up(n, 64); };
  SweepScratch s;
  s.logits = reinterpret_cast<float*>(scratch);
  s.dlogits = s.logits + seg(rows * G * C);
  s.row_loss = s.dlogits + seg(rows * G * C);
  s.row_correct = reinterpret_cast<int32_t*>(s.row_loss + seg(rows * G));
  s.partial = s.row_loss + 2 * seg(rows * G);
  s.floats = (s.partial - s.logits) + seg((int64_t)sweep_slices(rows) * G * sweep_hf(C, D));
  return s;
}

int64_t probe_sweep_scratch_bytes(int64_t rows, int dim, int C, int G) {
  if (dim % 4 != 0 || dim < 4 || dim > 1024 || C < 2 || C > HEAD_MAX_CLASSES || G < 1 || G > SW_MAX_HEADS || !sweep_rows_ok(rows, C, G))
    return -1;
  return sweep_scratch(nullptr, rows, dim, C, G).floats * (int64_t)sizeof(float);
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int launch_probe_sweep_head(const float* y, int64_t rows, int dim, const float* heads, int G, int C, const int64_t* labels, float* logits,
                            float* loss_out, int32_t* correct_out, float* head_grads, void* scratch, int64_t scratch_bytes, hipStream_t s) {
  const char* who = "mae_probe_sweep_head";
  MAE_REQUIRE(dim % 4 == 0 && dim >= 4 && dim <= 1024, "%s: dim = %d must be a multiple of 4 in [4, 1024]", who, dim);
  MAE_REQUIRE(C >= 2 && C <= HEAD_MAX_CLASSES, "%s: num_classes = %d outside [2, %d]", who, C, HEAD_MAX_CLASSES);
  MAE_REQUIRE(G >= 1 && G <= SW_MAX_HEADS, "%s: num_heads = %d outside [1, %d]", who, G, SW_MAX_HEADS);
  MAE_REQUIRE(sweep_rows_ok(rows, C, G), "%s: rows = %lld: need rows >= 1 and rows * num_heads * num_classes < 2^31",
              who, (long long)rows);
  MAE_REQUIRE(y && heads && scratch, "%s: y / heads / scratch is null", who);
  MAE_REQUIRE(labels || logits, "%s: without labels the call gives logits only and needs the logits buffer", who);
  MAE_REQUIRE(!labels || (loss_out && correct_out), "%s: labels need loss_out and correct_out", who);
  MAE_REQUIRE(!head_grads || labels, "%s: gradients need labels", who);
  MAE_REQUIRE(aligned16(y) && aligned16(heads) && aligned16(labels) && aligned16(logits) && aligned16(loss_out) && aligned16(correct_out) &&
              aligned16(head_grads) && aligned16(scratch), "%s: every buffer must be 16-byte aligned", who);
  const int64_t need = probe_sweep_scratch_bytes(rows, dim, C, G);
  MAE_REQUIRE(scratch_bytes >= need, "%s: scratch_bytes = %lld, mae_probe_sweep_scratch_bytes asks for %lld", who, (long long)scratch_bytes,
              (long long)need);
  const SweepScratch sc = sweep_scratch(scratch, rows, dim, C, G);
  const int NC = G * C, B = (int)rows;
  const int64_t HF = sweep_hf(C, dim);
  float* lg = logits ? logits : sc.logits;
  hipLaunchKernelGGL(sweep_fwd_kernel, dim3((unsigned)cdiv(B, SW_FR), (unsigned)cdiv(NC, SW_FC)), dim3(256), 0, s, y, B, dim, heads, C, NC, HF, lg);
  MAE_LAUNCH_CHECK();
  if (!labels) return 0;
  hipLaunchKernelGGL(sweep_softmax_kernel, dim3((unsigned)cdiv((int64_t)B * G, 4)), dim3(256), 0, s, (const float*)lg, B, C, G, labels, sc.row_loss,
                     sc.row_correct, head_grads ? sc.dlogits : (float*)nullptr);
  MAE_LAUNCH_CHECK();
  hipLaunchKernelGGL(sweep_reduce_kernel, dim3(G), dim3(256), 0, s, (const float*)sc.row_loss, (const int32_t*)sc.row_correct, B, loss_out, correct_out);
  MAE_LAUNCH_CHECK();
  if (!head_grads) return 0;
  const int S = sweep_slices(rows);
  hipLaunchKernelGGL(sweep_wgrad_kernel, dim3((unsigned)cdiv(NC, 128), (unsigned)cdiv(dim, SW_WD), S), dim3(256), 0, s, (const float*)sc.dlogits, y, B,
                     dim, C, NC, HF, G, sc.partial);
  MAE_LAUNCH_CHECK();
  return launch_sum_partials(sc.partial, S, (int)(G * HF), head_grads, nullptr, (int)(G * HF), s);
}

// ---------------------------------------------------------------------------------------------------
// LARS over G segments: lars_dev.cuh's blocks with the segment on blockIdx.y; lr and weight decay per segment ride in the arguments
// ---------------------------------------------------------------------------------------------------
struct LarsGroupHyper { float lr[SW_MAX_HEADS], wd[SW_MAX_HEADS]; };

__global__ void __launch_bounds__(256) lars_groups_sumsq_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t stride,
                                                                int64_t n4, int adapt, const LarsGroupHyper hy, float* __restrict__ scratch) {
  const int64_t o = (int64_t)blockIdx.y * stride;
  lars_sumsq_block(p + o, g + o, n4, adapt ? hy.wd[blockIdx.y] : 0.f, scratch + (int64_t)blockIdx.y * LARS_SCRATCH_FLOATS, blockIdx.x, gridDim.x);
}

__global__ void __launch_bounds__(256) lars_groups_finalize_kernel(float* __restrict__ scratch, int nb, float trust, float* __restrict__ norms_out) {
  float* sc = scratch + (int64_t)blockIdx.x * LARS_SCRATCH_FLOATS;
  lars_finalize_block(sc, nb, trust, sc + 2 * LARS_BLOCKS, norms_out ? norms_out + 2 * blockIdx.x : nullptr);
}

template <bool ADAPT>
__global__ void __launch_bounds__(256) lars_groups_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu,
                                                                 int64_t stride, int64_t n4, const LarsGroupHyper hy, float momentum,
                                                                 const float* __restrict__ scratch) {
  const int64_t o = (int64_t)blockIdx.y * stride;
  lars_update_block<ADAPT>(p + o, g + o, mu + o, n4, hy.lr[blockIdx.y], momentum, hy.wd[blockIdx.y],
                           scratch + (int64_t)blockIdx.y * LARS_SCRATCH_FLOATS + 2 * LARS_BLOCKS, blockIdx.x, gridDim.x);
}

int launch_lars_step_groups(float* p, const float* g, float* mu, int G, int64_t stride, int64_t n, int adapt, const float* lr, const float* wd,
                            float momentum, float trust, float* norms_out, float* scratch, int64_t scratch_floats, hipStream_t s) {
  const char* who = "mae_lars_step_groups";
  MAE_REQUIRE(G >= 1 && G <= SW_MAX_HEADS, "%s: num_groups = %d outside [1, %d]", who, G, SW_MAX_HEADS);
  MAE_REQUIRE(n >= 0 && n % 4 == 0 && stride % 4 == 0 && stride >= n, "%s: count = %lld and group_stride = %lld must be multiples of 4, stride >= count",
              who, (long long)n, (long long)stride);
  if (n == 0) return 0;
  MAE_REQUIRE(p && g && mu && lr && wd && scratch, "%s: params / grads / mu / lr / weight_decay / scratch is null", who);
  MAE_REQUIRE(aligned16(p) && aligned16(g) && aligned16(mu) && aligned16(scratch), "%s: params / grads / mu / scratch must be 16-byte aligned", who);
  MAE_REQUIRE(scratch_floats >= (int64_t)G * LARS_SCRATCH_FLOATS, "%s: scratch_floats = %lld, need %d per group", who, (long long)scratch_floats,
              LARS_SCRATCH_FLOATS);
  LarsGroupHyper hy = {};
  for (int i = 0; i < G; ++i) { hy.lr[i] = lr[i]; hy.wd[i] = wd[i]; }
  const int64_t n4 = n / 4;
  if (adapt || norms_out) {
    const int grid = lars_sum_grid(n4);
    hipLaunchKernelGGL(lars_groups_sumsq_kernel, dim3(grid, G), dim3(256), 0, s, (const float*)p, g, stride, n4, adapt, hy, scratch);
    MAE_LAUNCH_CHECK();
    hipLaunchKernelGGL(lars_groups_finalize_kernel, dim3(G), dim3(256), 0, s, scratch, grid, trust, norms_out);
    MAE_LAUNCH_CHECK();
  }
  const int grid = lars_update_grid(n4);
  with_bool(adapt != 0, [&](auto A) {
    hipLaunchKernelGGL((lars_groups_update_kernel<decltype(A)::value>), dim3(grid, G), dim3(256), 0, s, p, g, mu, stride, n4, hy, momentum,
                       (const float*)scratch);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

}  // namespace mae

extern "C" int64_t mae_probe_sweep_scratch_bytes(int64_t rows, int32_t dim, int32_t num_classes, int32_t num_heads) {
  return mae::probe_sweep_scratch_bytes(rows, dim, num_classes, num_heads);
}

extern "C" int mae_probe_sweep_head(const float* y, int64_t rows, int32_t dim, const float* heads, int32_t num_heads, int32_t num_classes,
                                    const int64_t* labels, float* logits, float* loss_out, int32_t* correct_out, float* head_grads, void* scratch,
                                    int64_t scratch_bytes, void* stream) {
  return mae::launch_probe_sweep_head(y, rows, dim, heads, num_heads, num_classes, labels, logits, loss_out, correct_out, head_grads, scratch,
                                      scratch_bytes, (hipStream_t)stream);
}

extern "C" int mae_lars_step_groups(float* params, const float* grads, float* mu, int32_t num_groups, int64_t group_stride, int64_t count,
                                    int32_t adapt, const float* lr, const float* weight_decay, float momentum, float trust_coefficient,
                                    float* norms_out, float* scratch, int64_t scratch_floats, void* stream) {
  return mae::launch_lars_step_groups(params, grads, mu, num_groups, group_stride, count, adapt, lr, weight_decay, momentum, trust_coefficient,
                                      norms_out, scratch, scratch_floats, (hipStream_t)stream);
}
