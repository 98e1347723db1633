// I-JEPA pieces that the MAE path does not have (BASELINE.json configs[2] and [4]).  The reference holds NO I-JEPA code
// ("JEPA" appears in README.md:1,9 and pyproject.toml:2 only): these kernels follow the specification written down in
// DESIGN.md from the I-JEPA paper (Assran et al. 2023: context encoder, EMA target encoder, narrow predictor fed with the
// context tokens plus one mask token per target position, latent regression loss), on the reference's own ViT pieces.
//   predictor_assemble(+bwd)  rows of the predictor input: nblk sequences per image = [k context tokens | m mask tokens],
//                             each with the position row of its token id
//   smooth_l1                 latent loss alternative to MSE (torch.nn.functional.smooth_l1_loss, beta = 1)
// All HBM-bound, a few hundred MB per launch at most.  (The row and token maps of this path are in k_index.hip.)
#include "kernels.h"

namespace mae {

// out[(b, blk, t)] = (t < k ? xdec[b*k + t] + pos[ctx[b][t]] : mask_token + pos[tgt[b][blk][t - k]])      fp32 rows of Dd
template <class T>
__global__ void __launch_bounds__(256) predictor_assemble_kernel(const T* __restrict__ xdec, const int32_t* __restrict__ ctx,
                                                                 const int32_t* __restrict__ tgt, const float* __restrict__ mask_token,
                                                                 const float* __restrict__ pos, int64_t rows, int k, int nblk, int m, int L,
                                                                 int D4, float* __restrict__ out) {
  const int rpb = 256 / D4, ro = threadIdx.x / D4, d = (threadIdx.x - ro * D4) * 4;
  if (ro >= rpb) return;
  const int Tq = k + m;
  for (int64_t r = (int64_t)blockIdx.x * rpb + ro; r < rows; r += (int64_t)gridDim.x * rpb) {
    const int seq = (int)((uint32_t)r / (uint32_t)Tq);  // rows < 2^31 is checked by the launcher
    const int t = (int)(r - (int64_t)seq * Tq);
    const int b = seq / nblk;
    int tokid;
    f32x4 v;
    if (t < k) { tokid = ctx[(int64_t)b * k + t]; v = load4(xdec + ((int64_t)b * k + t) * (D4 * 4) + d); }
    else { tokid = tgt[(int64_t)seq * m + (t - k)]; v = load4(mask_token + d); }
    tokid = tokid < 0 ? 0 : (tokid >= L ? L - 1 : tokid);  // ids are range-checked on the host; never fault here
    v += load4(pos + (int64_t)tokid * (D4 * 4) + d);
    store4_nt(out + r * (D4 * 4) + d, v);
  }
}
int launch_predictor_assemble(const void* xdec, int dt, const int32_t* ctx32, const int32_t* tgt32, const float* mask_token, const float* pos,
                              int B, int k, int nblk, int m, int L, int Dd, float* out, hipStream_t s) {
  MAE_REQUIRE(xdec && ctx32 && tgt32 && mask_token && pos && out && Dd % 4 == 0 && Dd / 4 <= 256, "predictor_assemble: bad arguments");
  const int64_t rows = (int64_t)B * nblk * (k + m);
  MAE_REQUIRE(rows < (1ll << 31), "predictor_assemble: B * nblk * (k + m) < 2^31");
  const int grid = (int)std::min<int64_t>(cdiv(rows, 256 / (Dd / 4)), 256 * 16);
  with_dtype(dt, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(predictor_assemble_kernel<T>, dim3(grid), dim3(256), 0, s, (const T*)xdec, ctx32, tgt32, mask_token, pos, rows, k, nblk, m, L, Dd / 4, out);
  });
  MAE_LAUNCH_CHECK();
  return 0;
}

// adjoint: d_xdec[b*k + t] = sum over the nblk copies of context row t; partial[block] = column sums of the mask-token rows.  The
// split kernels' block frame (split_block, kernels.h) around two loops of its own: one sums nblk rows of dx per context row, the
// other finds the mask-token rows through (sequence, j)
template <class T>
__global__ void __launch_bounds__(256) predictor_assemble_bwd_kernel(const float* __restrict__ dx, int64_t ctx_rows, int k, int nblk, int m,
                                                                     int D, T* __restrict__ d_xdec, float* __restrict__ partial) {
  split_block(D, partial, [&](int RPI, int ro, int d0, f32x4& acc) {
    const int Tq = k + m;
    // context rows: r = b*k + t
    for (int64_t r = (int64_t)blockIdx.x * RPI + ro; r < ctx_rows; r += (int64_t)gridDim.x * RPI) {
      const int64_t b = r / k;
      const int t = (int)(r - b * k);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      for (int blk = 0; blk < nblk; ++blk) v += load4(dx + ((b * nblk + blk) * Tq + t) * (int64_t)D + d0);
      store4(d_xdec + r * D + d0, v);
    }
    // mask-token rows: q = seq*m + j
    const int64_t mask_rows = (ctx_rows / k) * nblk * m;
    for (int64_t q = (int64_t)blockIdx.x * RPI + ro; q < mask_rows; q += (int64_t)gridDim.x * RPI) {
      const int64_t seq = q / m;
      acc += load4(dx + (seq * Tq + k + (q - seq * m)) * (int64_t)D + d0);
    }
  });
}
int launch_predictor_assemble_bwd(const float* dx, int B, int k, int nblk, int m, int Dd, int dt, void* d_xdec, float* d_mask_token,
                                  float* partial, hipStream_t s) {
  MAE_REQUIRE(dx && d_xdec && d_mask_token && partial && Dd % 4 == 0 && Dd <= 1024, "predictor_assemble_bwd: bad arguments");
  const int64_t ctx_rows = (int64_t)B * k;
  return launch_split(std::max<int64_t>(ctx_rows, (int64_t)B * nblk * m), Dd, dt, partial, d_mask_token, s, [&](auto t, dim3 grid, size_t lds) {
    using T = decltype(t);
    hipLaunchKernelGGL(predictor_assemble_bwd_kernel<T>, grid, dim3(256), lds, s, dx, ctx_rows, k, nblk, m, Dd, (T*)d_xdec, partial);
  });
}

// smooth L1 (beta = 1): mean over n of (|d| < 1 ? 0.5 d^2 : |d| - 0.5); d_pred = grad_scale * clamp(d, -1, 1) / n
template <class T, bool HAS_GRAD>
__global__ void __launch_bounds__(256) smooth_l1_kernel(const float* __restrict__ pred, const float* __restrict__ target, int64_t n4, float gscale,
                                                        float* __restrict__ partial, T* __restrict__ dpred) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t i = blockIdx.x * 256ll + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const f32x4 d = load4(pred + i * 4) - load4(target + i * 4);
    f32x4 g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = fabsf(d[j]);
      acc += a < 1.0f ? 0.5f * d[j] * d[j] : a - 0.5f;
      g[j] = fminf(fmaxf(d[j], -1.0f), 1.0f) * gscale;
    }
    if (HAS_GRAD) store4(dpred + i * 4, g);
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
int launch_smooth_l1(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, void* d_pred, int dpred_dt,
                     float* scratch, hipStream_t s) {
  MAE_REQUIRE(pred && target && loss && scratch && n > 0 && n % 4 == 0, "smooth_l1: need n %% 4 == 0 and non-null buffers");
  const int64_t n4 = n / 4;
  const int grid = (int)std::min<int64_t>(cdiv(n4, 256), RED_BLOCKS);
  const float gs = grad_scale / (float)n;
  MAE_LAUNCH_LOSS(smooth_l1_kernel, (), grid, 0, s, d_pred, dpred_dt, scratch, 1.0f / (float)n, loss, pred, target, n4, gs);
  return 0;
}

}  // namespace mae

extern "C" int mae_predictor_assemble(const void* xdec, int32_t dtype, const int32_t* ctx32, const int32_t* tgt32, const float* mask_token,
                                      const float* pos, int32_t batch, int32_t num_context, int32_t num_blocks, int32_t block_tokens,
                                      int32_t seq_len, int32_t dim, float* out, void* stream) {
  MAE_REQUIRE(batch > 0 && num_context > 0 && num_blocks > 0 && block_tokens > 0 && seq_len > 0, "mae_predictor_assemble: bad arguments");
  return mae::launch_predictor_assemble(xdec, dtype, ctx32, tgt32, mask_token, pos, batch, num_context, num_blocks, block_tokens, seq_len, dim, out,
                                        (hipStream_t)stream);
}

extern "C" int mae_predictor_assemble_bwd(const float* dx, int32_t batch, int32_t num_context, int32_t num_blocks, int32_t block_tokens, int32_t dim,
                                          int32_t dtype, void* d_xdec, float* d_mask_token, float* partial, void* stream) {
  MAE_REQUIRE(batch > 0 && num_context > 0 && num_blocks > 0 && block_tokens > 0, "mae_predictor_assemble_bwd: bad arguments");
  return mae::launch_predictor_assemble_bwd(dx, batch, num_context, num_blocks, block_tokens, dim, dtype, d_xdec, d_mask_token, partial,
                                            (hipStream_t)stream);
}

extern "C" int mae_smooth_l1_loss(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, void* d_pred,
                                  int32_t d_pred_dtype, float* scratch, void* stream) {
  return mae::launch_smooth_l1(pred, target, n, grad_scale, loss, d_pred, d_pred_dtype, scratch, (hipStream_t)stream);
}
