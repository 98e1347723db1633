// Internal launch API of libmae_hip.so: one function per kernel family.  Every function validates its
// operand shapes on the host before launching and returns 0 / non-zero (message via mae_last_error()).
#pragma once
#include "common.cuh"

namespace mae {

// ---- k_index.hip: masks and token-index maps ---------------------------------------------------
// noise (B, L) -> ascending-noise permutation with column 0 forced first; any output may be null.
int launch_mask_from_noise(const float* noise, int B, int L, int k, int64_t* keep64, int64_t* mask64,
                           int32_t* keep32, int32_t* mask32, hipStream_t s);
int launch_idx_to_i32(const int64_t* src, int32_t* dst, int64_t n, hipStream_t s);
// inv[b][t] = j with keep[b][j] == t, else -1
int launch_build_inverse(const int32_t* keep32, int B, int k, int L, int32_t* inv, hipStream_t s);
// rows[b*m + j] = b*L + mask[b][j]  (row map of the masked tokens inside the (B*L) decoder matrix)
int launch_build_row_map(const int32_t* idx32, int B, int n_per, int L, int32_t* rows, hipStream_t s);
int launch_iota_tokens(int32_t* keep32, int B, int N, int first, hipStream_t s);      // keep[b][j] = first + j: N tokens of every image
int launch_fill(float* p, float v, int64_t n, hipStream_t s);
int launch_build_tail_row_map(int seqs, int T, int m, int32_t* rows, hipStream_t s);  // last m rows of every sequence of T
int launch_rows_from_tokens(const int32_t* tok, int B, int per_image, int N, int32_t* rows, hipStream_t s);  // b*N + tok-1

// ---- k_patch.hip: token rows <-> sequences ----------------------------------------------------------
// in place on x (B*k, D) fp32: x[r] = (t == 0 ? cls : x[r]) + pos[t]
int launch_assemble_visible(float* x, const int32_t* tok, const float* cls, const float* pos, int64_t rows, int D,
                            hipStream_t s);
// dtok (dt) = dx with class-token rows zeroed; dcls[D] = sum of class-token rows.  partial: >= 512*D floats
int launch_visible_grad_split(const float* dx, const int32_t* tok, int64_t rows, int D, int dt, void* dtok,
                              float* dcls, float* partial, hipStream_t s);
// out[b][t] = (inv[b][t] >= 0 ? xdec[b*k + inv] : mask_token) + pos[t]   (fp32 out)
int launch_decoder_assemble(const void* xdec, int dt, const int32_t* inv, const float* mask_token, const float* pos,
                            int B, int k, int L, int Dd, float* out, hipStream_t s);
// d_xdec[b*k+j] (dt) = dx[b][keep[b][j]];  d_mask_token[Dd] = sum over rows with inv < 0.  partial: >= 512*Dd floats
int launch_decoder_assemble_bwd(const float* dx, const int32_t* inv, int B, int k, int L, int Dd, int dt, void* d_xdec,
                                float* d_mask_token, float* partial, hipStream_t s);
// The row clear: +0.0 in every row of dres (fp32) / dres_c (act) that is not kept.  zero_unpredicted_rows keeps the rows with
// inv[row] < 0, or (inv == nullptr) the last m rows of every sequence of Tseq; zero_token_rows keeps row 0 of every sequence of L
int launch_zero_unpredicted_rows(const int32_t* inv, int64_t rows, int Tseq, int m, int D, int act, float* dres, void* dres_c, hipStream_t s);
int launch_zero_token_rows(int64_t rows, int L, int D, int act, float* dres, void* dres_c, hipStream_t s);
int launch_cast(const void* src, int src_dt, void* dst, int dst_dt, int64_t n, hipStream_t s);
// out[r] = x[r] + pos[r mod L] (fp32 rows of D)
int launch_add_rows_pos(const float* x, const float* pos, int64_t rows, int L, int D, float* out, hipStream_t s);
// dst (dt) += src (fp32)
int launch_add_into(const float* src, void* dst, int dst_dt, int64_t n, hipStream_t s);
// out[c] = sum_{i<G} partial[i][c] in row order (deterministic); columns [0,split) go to out0, [split,C) to out1
int launch_sum_partials(const float* partial, int G, int C, float* out0, float* out1, int split, hipStream_t s);

// The "split" kernels (visible_grad_split, decoder_assemble_bwd; predictor_assemble_bwd of k_jepa.hip) walk a (rows, D) fp32 matrix
// alike: thread (ro, d0) owns 4 columns of row offset ro, a block covers RPI = 256 / (D/4) rows per trip and at most SPLIT_BLOCKS
// blocks stride the matrix.  walk(RPI, ro, d0, acc) is the kernel's own part: it adds the rows it selects into the thread's column
// sum.  The sums are then added over ro through LDS ([RPI][D] floats, dynamic) into partial[block][D]; launch_sum_partials adds
// the blocks.
constexpr int SPLIT_BLOCKS = 512;
template <class Walk>
__device__ __forceinline__ void split_block(int D, float* __restrict__ partial, Walk walk) {
  extern __shared__ __attribute__((aligned(16))) float red[];  // [RPI][D]
  const int D4 = D / 4, RPI = 256 / D4;
  const int ro = threadIdx.x / D4, d0 = (threadIdx.x - ro * D4) * 4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (ro < RPI) {
    walk(RPI, ro, d0, acc);
    store4(red + ro * D + d0, acc);
  }
  __syncthreads();
  if (ro == 0) {
    for (int i = 1; i < RPI; ++i) acc += load4(red + i * D + d0);
    store4(partial + (int64_t)blockIdx.x * D + d0, acc);
  }
}
// launcher tail of a split kernel over `rows` rows: launch(T{}, grid, lds) launches it on s, then out[D] = sum of the partials
template <class L>
int launch_split(int64_t rows, int D, int dt, float* partial, float* out, hipStream_t s, L launch) {
  const int RPI = 256 / (D / 4);
  const int G = (int)std::min<int64_t>(cdiv(rows, RPI), SPLIT_BLOCKS);
  with_dtype(dt, [&](auto t) { launch(t, dim3(G), (size_t)RPI * D * sizeof(float)); });
  MAE_LAUNCH_CHECK();
  return launch_sum_partials(partial, G, D, out, nullptr, D, s);
}

// ---- k_jepa.hip: I-JEPA predictor input, its adjoint and the latent loss (no reference code: spec in DESIGN.md) ---------------
int launch_predictor_assemble(const void* xdec, int dt, const int32_t* ctx32, const int32_t* tgt32, const float* mask_token, const float* pos,
                              int B, int k, int nblk, int m, int L, int Dd, float* out, hipStream_t s);
int launch_predictor_assemble_bwd(const float* dx, int B, int k, int nblk, int m, int Dd, int dt, void* d_xdec, float* d_mask_token,
                                  float* partial, hipStream_t s);
int launch_smooth_l1(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, void* d_pred, int dpred_dt,
                     float* scratch, hipStream_t s);

// ---- k_pixels.hip: the three readers of the image; images are fp32 (normalised) or uint8 (img_dt = MAE_F32 / MAE_U8), uint8 with
// ToTensor + Normalize(.5,.5) fused into the read.  uint8 images, and the loss on float images where the geometry allows, go through
// the band walk (one workgroup streams one row of patches into LDS); float images otherwise through per-pixel gathers ---------------
// A[(b,j)][c*p*p + py*p + px] = images[b][c][ph*p+py][pw*p+px] for token t = tok[b][j] >= 1 (patch t-1), zeros for t == 0
int launch_gather_patches(const void* images, int img_dt, const int32_t* tok, int B, int k, int C, int img, int p, int dt, void* out,
                          hipStream_t s);
// target (B*m, P) fp32 in (py, px, c) order for patch clamp(idx[b][j]-1, 0, g*g-1); idx is int64 when idx64 != 0, else int32
int launch_patchify_gather(const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p, float* target,
                           hipStream_t s);
// launch_mse with that target read straight from the image (never materialised).  Float images: path 0 = band walk where it applies
// (MAE_MSE_BAND=0 switches it off), else the per-pixel gather; path 1 = the gather alone
int launch_mse_from_images(const float* pred, const void* images, int img_dt, const int32_t* mask32, int B, int m, int C, int img, int p,
                           float grad_scale, float* loss, void* d_pred, int dpred_dt, float* scratch, int path, hipStream_t s);
int launch_augment_crop_flip_u8(const uint8_t* in, const int32_t* params, int B, int C, int S, uint8_t* out, hipStream_t s);

// ---- k_classifier.hip: pooled linear head + cross-entropy, full-sequence embedding gradient ---------------------------------
constexpr int HEAD_MAX_CLASSES = 128;   // classes held in LDS by the head kernel
constexpr int CLS_WGRAD_SLICES = 64;    // batch slices of the head weight-gradient partials
constexpr int CLS_EMBED_SLICES = 64;    // batch slices of the d pos_embed partials
// soft targets of the head: t[c] = eps / C + (1 - eps) * (lam[b] * [c == labels[b]] + (1 - lam[b]) * [c == labels_b[b]]);
// labels_b null = labels, lam (device, B floats) null = 1.  Nothing active = the hard-label kernels, launched as before.
struct HeadSoft {
  const int64_t* labels_b;
  const float* lam;
  float eps;
  bool active() const { return labels_b || lam || eps != 0.f; }
};
// The pool rules every caller of the head shares: with_cls 0 or 1, a known pool, and MAE_POOL_CLS only on a sequence with a class
// token.  extended = false is a first-generation entry point: [cls | patches] with MAE_POOL_CLS or MAE_POOL_MEAN, nothing else.
int check_pool(int with_cls, int pool, bool extended, const char* who);
// One head call.  feats is (B * seq, D) in dt; logits = pooled W^T + bias; row loss / correct flag per image; loss_out = mean of
// the row losses, correct_out = number of correct rows (fixed-order reduction; either may be null).
//   with dlogits_out: d_logits and pooled (both fp32, rounded at the bf16 points);
//   with dfeat_out:   MAE_POOL_CLS -> (B, D) compact d_pooled, a mean -> (B * seq, D): d_pooled / rows on the pooled rows, exact
//                     zeros on the others;
//   with cls_rows:    (MAE_POOL_CLS) the class-row map and the rows' LayerNorm statistics, compact.
// Two kernels, two summation orders: MAE_POOL_CLS and the all-row mean behind a class token take one block per image with each
// thread walking the rows serially; a patch-only sequence or MAE_POOL_MEAN_PATCHES pools rows [with_cls, seq) with four waves
// loading rows and their partial sums added through LDS.
struct HeadCall {
  const void* feats = nullptr;
  int dt = MAE_F32, B = 0, seq = 0, D = 0, with_cls = 1, pool = MAE_POOL_CLS, C = 0;
  const float *W = nullptr, *bias = nullptr;
  const int64_t* labels = nullptr;
  HeadSoft soft = {nullptr, nullptr, 0.f};
  float grad_scale = 1.f;
  float *logits_out = nullptr, *row_loss = nullptr, *loss_out = nullptr, *pooled_out = nullptr, *dlogits_out = nullptr;
  int32_t *row_correct = nullptr, *correct_out = nullptr, *cls_rows = nullptr;
  void* dfeat_out = nullptr;
  const float *mean_all = nullptr, *rstd_all = nullptr;  // class-row statistics: every row's, read ...
  float *mean_c = nullptr, *rstd_c = nullptr;            // ... and one per image, written
  bool range() const { return !with_cls || pool == MAE_POOL_MEAN_PATCHES; }
};
int launch_classifier_head(const HeadCall& h, hipStream_t s);
// head_grads[0 .. C*D) = dW, [C*D .. C*D+C) = db; partial >= classifier_wgrad_partial_floats, sum_out >= round_up(C*D+C, 4) floats
int64_t classifier_wgrad_partial_floats(int B, int C, int D);
int launch_classifier_head_wgrad(const float* dlogits, const float* pooled, int B, int C, int D, float* partial, float* sum_out,
                                 float* head_grads, hipStream_t s);
// one read of dx (B, L, D), L rows per image.  has_cls: dtok = dx with class rows zeroed, dpos (L*D) = sum over images, dcls (D) =
// dpos[0].  Patch-only (row t is patch token t + 1): dtok = dx, dpos ((L + 1) * D) rows 1..L = sum over images, dpos row 0 and
// dcls = exact zeros.  partial >= full_grad_split_slices(B, L, D) * L * D floats
int full_grad_split_slices(int B, int L, int D);
int launch_full_grad_split(const float* dx, int B, int L, int D, int dt, void* dtok, float* dpos, float* dcls, float* partial, bool has_cls,
                           hipStream_t s);

// ---- k_representation.hip: frozen-encoder features and the k-NN probe -----------------------------------------------------
// out + b * out_stride (fp32, W floats) = the pool (with_cls, pool) names over the rows of LN(x_mid + branch) of image b (seq rows each),
// then f / (||f|| + 1e-8) when normalize == MAE_FEAT_L2: (B, D), or one slice of a (B, taps, W) buffer.  W = features_tap_width: D, or
// 2 D for MAE_POOL_CLS_MEAN_PATCHES = [class row | patch mean].  Reads only the pooled rows; out needs 4-byte alignment only.
int features_tap_width(int pool, int D);
int launch_features_tap(const float* x_mid, const void* branch, int branch_dt, const float* gamma, const float* beta, float eps, int B, int seq,
                        int D, int with_cls, int pool, int normalize, float* out, int64_t out_stride, hipStream_t s);
// top-k of queries (Q, D) . bank (N, D)^T per query row: similarity descending, bank index ascending; -1 for bad arguments
int knn_splits(int64_t Q, int64_t N, int k);
int64_t knn_scratch_bytes(int64_t Q, int64_t N, int D, int k);
int launch_knn_topk(const float* queries, int64_t Q, const float* bank, int64_t N, int D, int k, float* topk_sim, int64_t* topk_idx,
                    void* scratch, int64_t scratch_bytes, hipStream_t s);
int launch_knn_vote(const float* sim, const int64_t* idx, int64_t Q, int k_stride, int k, const int64_t* labels, int C, float T, float* scores,
                    int64_t* pred, hipStream_t s);

// ---- k_reconstruct.hip: MAE reconstruction compose (inverse of patchify_gather) + whole-image error sums ---------------------
// recon / masked (B, C, S, S) in out_dt and stats (B, 2) = {sum d^2, sum |d|} from images, pred (B, m, p*p*C) and idx_mask (int64);
// any of the three outputs may be null.  check_ validates everything on the host and launches nothing.
int64_t reconstruct_scratch_bytes(int B, int C, int S, int p);
int check_reconstruct_compose(const void* images, int img_dt, const float* pred, const int64_t* idx_mask, int B, int C, int S, int p, int m,
                              int out_dt, const void* recon, const void* masked, const float* stats, const void* scratch,
                              int64_t scratch_bytes);
int launch_reconstruct_compose(const void* images, int img_dt, const float* pred, const int64_t* idx_mask, int B, int C, int S, int p, int m,
                               float fill, int out_dt, void* recon, void* masked, float* stats, void* scratch, int64_t scratch_bytes,
                               hipStream_t s);

// ---- k_mix.hip: mixup / CutMix of a batch with its partner images ------------------------------------------------------------
// out[b] = box ? partner pixel : lam[b] * own + (1 - lam[b]) * partner (MAE_F32 out), or the byte select alone (MAE_U8 out)
int launch_mix_batch(const void* images, int img_dt, const int32_t* partner, const float* lam, const int32_t* box, int B, int C, int S,
                     int out_dt, void* out, hipStream_t s);

// ---- k_augment.hip: crop / flip, RandAugment ops and random erasing of one image per workgroup, the image held in LDS ----------
int launch_augment_ops_u8(const uint8_t* images, int B, int C, int S, const int32_t* op_codes, const double* op_args, int num_ops,
                          const int32_t* erase, int out_dt_flags, void* out, hipStream_t s);

// ---- k_resize.hip: (B, C, Si, Si) -> (B, C, So, So) through a crop box and a flip per image (params (B, 5) or null: whole image) ----
// bilinear where an axis keeps or gains pixels, the antialiasing triangle filter where it loses them; u8 -> u8 | f32, f32 -> f32
int launch_resize_crop_flip(const void* images, int in_dt, int B, int C, int Si, const int32_t* params, int So, int out_dt, void* out,
                            hipStream_t s);

// ---- k_normpix.hip: targets standardised per patch (norm_pix_loss); idx is int64 when idx64 != 0, else int32 ---------------------
// mae_mse_loss with the target (x - mean) * rstd of the image's patches, never materialised; stage-1 partials in scratch (1024+ floats)
int launch_mse_norm_pix(const float* pred, const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p,
                        float grad_scale, float* loss, void* d_pred, int dpred_dt, float* scratch, hipStream_t s);
// the materialised target (B*m, P) and, optionally, each row's mean / rstd
int launch_patchify_gather_norm(const void* images, int img_dt, const void* idx, int idx64, int B, int m, int C, int img, int p, float* target,
                                float* mean, float* rstd, hipStream_t s);
// out = pred * sqrt(var + eps) + mean (out may be pred)
int launch_norm_pix_restore(const void* images, int img_dt, const float* pred, const void* idx, int idx64, int B, int m, int C, int img, int p,
                            float* out, hipStream_t s);

// ---- k_probe.hip: the linear probe's BatchNorm1d(affine=False) over feature rows and the LARS step of its head --------------------
// y = (x - mean) rsqrt(var + eps) per column: training != 0 takes the batch statistics (centred, two column reductions into
// partials + launch_sum_partials) and updates the running buffers (may both be null); else the running buffers give them.
// y may be x.  scratch >= batchnorm_scratch_bytes (-1 = outside the limits); mean_out / rstd_out (dim) may be null
int64_t batchnorm_scratch_bytes(int64_t rows, int dim);
int launch_batchnorm_fwd(const float* x, int64_t rows, int dim, float eps, int training, float momentum, float* running_mean,
                         float* running_var, float* y, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, hipStream_t s);
// the statistics half of launch_batchnorm_fwd: the same device code, so mean_out / rstd_out / the running buffers get the same bits;
// no normalising sweep and no y.  mean_out and rstd_out are required
int launch_batchnorm_stats(const float* x, int64_t rows, int dim, float eps, int training, float momentum, float* running_mean,
                           float* running_var, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, hipStream_t s);
// dp = adapt ? (g + wd p) q : g, q = trust |p| / |g + wd p| (1 where a norm is 0); mu = momentum mu + dp; p -= lr mu.
// norms_out (2 floats, may be null) = |p|, |g + wd p|.  scratch >= 4096 floats
int launch_lars_step(float* p, const float* g, float* mu, int64_t n, int adapt, float lr, float momentum, float wd, float trust,
                     float* norms_out, float* scratch, hipStream_t s);

// ---- k_probe_sweep.hip: G probe heads on the same BatchNorm output in one pass, and LARS over G segments -----------
// heads (G, HF = round_up(C D + C, 4)): [W (C, D) | b (C) | padding] per head.  logits (G, rows, C), loss_out / correct_out (G),
// head_grads (G, HF); the bits of head g do not depend on G or on g.  scratch >= probe_sweep_scratch_bytes (-1 = outside the limits)
int64_t probe_sweep_scratch_bytes(int64_t rows, int dim, int C, int G);
int launch_probe_sweep_head(const float* y, int64_t rows, int dim, const float* heads, int G, int C, const int64_t* labels, float* logits,
                            float* loss_out, int32_t* correct_out, float* head_grads, void* scratch, int64_t scratch_bytes, hipStream_t s);
// launch_lars_step on the G segments p + g stride of n elements each, bit for bit; lr / wd are host arrays of G floats that travel in
// the kernel arguments.  norms_out (G, 2) may be null.  scratch >= 4096 G floats
int launch_lars_step_groups(float* p, const float* g, float* mu, int G, int64_t stride, int64_t n, int adapt, const float* lr, const float* wd,
                            float momentum, float trust, float* norms_out, float* scratch, int64_t scratch_floats, hipStream_t s);

// ---- k_tsne.hip: exact t-SNE in the plane, 8 <= n <= 16384; fp32, fixed orders, no atomics -------------------------
// P is (n, tsne_pitch(n) = round_up(n, 4)) with zeros in the padding columns; -1 outside the limits
int tsne_pitch(int n);
int64_t tsne_scratch_bytes(int n, int dim);   // the gradient's scratch
// x (n, dim) -> symmetric joint P; sqdist (n, n), beta (n), p_cond (n, n) optional.  The P buffer is the only working space
int launch_tsne_affinities(const float* x, int n, int dim, float perplexity, float* P, float* sqdist, float* beta, float* p_cond, hipStream_t s);
// grad (n, 2) = 4 (alpha a - r / Z) in one pass over P; kl (1 float, may be null) = sum p (log p - log w) + log Z
int launch_tsne_gradient(const float* P, const float* y, int n, float alpha, float* grad, float* kl, void* scratch, int64_t scratch_bytes,
                         hipStream_t s);
// sklearn's _gradient_descent step on (y, update, gains), every operation rounded once
int launch_tsne_update(float* y, float* upd, float* gains, const float* grad, int n, float momentum, float lr, float min_gain, hipStream_t s);
// both, the step inside the gradient's finalising launch: the bits of launch_tsne_gradient followed by launch_tsne_update
int launch_tsne_step(const float* P, float* y, float* upd, float* gains, int n, float alpha, float momentum, float lr, float min_gain, float* grad,
                     float* kl, void* scratch, int64_t scratch_bytes, hipStream_t s);

// ---- k_umap.hip: UMAP in the plane, 8 <= n <= 16384, 2 <= k <= 64, k < n; fp32, fixed orders, no atomics -------------
int64_t umap_scratch_bytes(int n, int dim, int k);   // the squared distances and two rows of floats; -1 outside the limits
// x (n, dim) -> the k nearest rows of every row (itself included) by (distance, index), umap-learn's rho, sigma and memberships
int launch_umap_fuzzy_knn(const float* x, int n, int dim, int k, int32_t* knn_idx, float* knn_dist, float* memb, float* rho, float* sigma, void* scratch,
                          int64_t scratch_bytes, hipStream_t s);
// one synchronous layout epoch over the CSR graph (row_ptr, col, eps, next): y_out from y_in, next += eps on the edges that fired
int launch_umap_epoch(const float* y_in, float* y_out, const int32_t* row_ptr, const int32_t* col, const float* eps, float* next, int n, float a, float b,
                      float gamma, float alpha, int t, int rate, uint32_t seed, hipStream_t s);

// ---- k_attnpool.hip: the attentive probe's pool over cached tokens and the small products around it -------------
// x (B, T, D) fp32 tokens, centred on load with mean (D, null = 0); uq (H, D).  ybar[b][h] = sum_t a (x - mean), a = softmax_t of
// (x - mean) . uq[h]; lse (B, H) = the log of the softmax denominator.  One workgroup per image, online softmax over token chunks
int launch_attn_pool_fwd(const float* x, const float* mean, const float* uq, int64_t B, int64_t T, int D, int H, float* ybar, float* lse,
                         hipStream_t s);
// duq[h] = sum_{b,t} a (da - delta) (x - mean), da = (x - mean) . g[b][h], delta = ybar[b][h] . g[b][h]; image slices into scratch
// (attn_pool_bwd_scratch_bytes, -1 outside the limits), added by launch_sum_partials
int64_t attn_pool_bwd_scratch_bytes(int64_t B, int64_t T, int D, int H);
int launch_attn_pool_bwd(const float* x, const float* mean, const float* uq, const float* lse, const float* ybar, const float* g, int64_t B,
                         int64_t T, int D, int H, float* duq, void* scratch, int64_t scratch_bytes, hipStream_t s);
// uq = rstd * (hd^-1/2 Wk[h]^T q[h]) and its adjoint: dwk[n] = hd^-1/2 q[n] (rstd duq[h]), dq[n] = hd^-1/2 Wk[n] . (rstd duq[h])
int launch_attn_probe_fold(const float* q, const float* wk, const float* rstd, int D, int H, float* uq, hipStream_t s);
int launch_attn_probe_fold_bwd(const float* duq, const float* q, const float* wk, const float* rstd, int D, int H, float* dq, float* dwk,
                               hipStream_t s);
// p[b][n] = sum_d (Wv[n][d] rstd[d]) ybar[b][h(n)][d] and its adjoints: g[b][h] = rstd * (Wv[h]^T dp[b][h]),
// dwv[n] = rstd * sum_b dp[b][n] ybar[b][h(n)] (batch slices into scratch, added by launch_sum_partials)
int launch_attn_probe_project(const float* ybar, const float* rstd, const float* wv, int64_t B, int D, int H, float* p, hipStream_t s);
int64_t attn_probe_project_bwd_scratch_bytes(int64_t B, int D, int H);
int launch_attn_probe_project_bwd(const float* dp, const float* ybar, const float* rstd, const float* wv, int64_t B, int D, int H, float* g,
                                  float* dwv, void* scratch, int64_t scratch_bytes, hipStream_t s);

// ---- k_loss_optim.hip -----------------------------------------------------------------------------
// loss[0] = mean((pred-target)^2); d_pred (dt, may be null) = grad_scale*2*(pred-target)/n.  scratch >= 1024+ floats
int launch_mse(const float* pred, const float* target, int64_t n, float grad_scale, float* loss, void* d_pred,
               int dpred_dt, float* scratch, hipStream_t s);
// out[0] = inv_n * sum of partial[0 .. nb): the second stage of the loss reductions
int launch_mean_finalize(const float* partial, int nb, float inv_n, float* out, hipStream_t s);
// Every loss runs in two stages.  Stage 1 is a kernel family K<.., T, HAS_GRAD> whose arguments end in (float* partial, T* dpred): the
// instantiation that d_pred asks for (null: <float, false>, else <bf16, true> or <float, true>) leaves `grid` <= RED_BLOCKS block sums
// in scratch (RED_BLOCKS floats + 8); stage 2 is launch_mean_finalize.  PRE holds the family's leading template arguments with their
// comma, in parentheses: () or (uint8_t,).  `...` are the kernel's arguments in front of (scratch, d_pred).
constexpr int RED_BLOCKS = 1024;  // stage-1 partial count upper bound of every scalar sum (the losses, the gradient's sum of squares)
template <class K, class T, class... A>
int launch_loss_stage1(K kernel, int grid, size_t lds, hipStream_t s, T* dpred, A... args) {
  MAE_TRY(allow_lds(kernel, lds));
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, s, args..., dpred);
  MAE_LAUNCH_CHECK();
  return 0;
}
#define MAE_UNPAREN(...) __VA_ARGS__
#define MAE_LAUNCH_LOSS(K, PRE, grid, lds, s, d_pred, dpred_dt, scratch, inv_n, loss, ...)                                                     \
  do {                                                                                                                                        \
    if (!(d_pred)) MAE_TRY((launch_loss_stage1(K<MAE_UNPAREN PRE float, false>, grid, lds, s, (float*)nullptr, __VA_ARGS__, scratch)));       \
    else if ((dpred_dt) == MAE_BF16) MAE_TRY((launch_loss_stage1(K<MAE_UNPAREN PRE bf16, true>, grid, lds, s, (bf16*)(d_pred), __VA_ARGS__, scratch))); \
    else MAE_TRY((launch_loss_stage1(K<MAE_UNPAREN PRE float, true>, grid, lds, s, (float*)(d_pred), __VA_ARGS__, scratch)));                 \
    MAE_TRY(launch_mean_finalize(scratch, grid, inv_n, loss, s));                                                                             \
  } while (0)
// stats[0] = ||g||_2, stats[1] = min(1, max_norm/(norm+1e-6)).  scratch >= 1024+ floats
int launch_grad_norm(const float* g, int64_t n, float max_norm, float* stats, float* scratch, hipStream_t s);
int launch_grad_sumsq(const float* g, int64_t n, float* out, float* scratch, hipStream_t s);
// io[0] += sum(g^2) (io[1] is a temporary)
int launch_grad_sumsq_accumulate(const float* g, int64_t n, float* io, float* scratch, hipStream_t s);
int launch_clip_from_sumsq(const float* sumsq, float max_norm, float* stats, hipStream_t s);
// AdamW with g scaled by stats[1]; optionally refresh bf16 copy of the params (wbf may be null)
// ema_target != null: target[0 .. ema_n) = ema_momentum * target + (1 - ema_momentum) * p_new in the same sweep (+ its bf16 copy)
int launch_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps,
                 float wd, float bc1, float bc2, const float* stats, bf16* wbf, hipStream_t s, float* ema_target = nullptr,
                 bf16* ema_wbf = nullptr, int64_t ema_n = 0, float ema_momentum = 0.f);
// dst[0 .. n) = (overwrite ? 0 : dst) + src: one fp32 add per element, no atomics (gradient accumulation over micro-batches)
constexpr int GRAD_ACC_BLOCKS = 2048;  // grid cap of the sweep; MAE_GRAD_ACC_BLOCKS of mae_hip.h and GRAD_ACC_BLOCKS of _lib.py
int launch_grad_accumulate(float* dst, const float* src, int64_t n, bool overwrite, hipStream_t s);
int launch_f32_to_bf16(const float* src, bf16* dst, int64_t n, hipStream_t s);
// dst[c][r] = (bf16) src[r][c] for a whole list of matrices living in one arena (one launch); passed by value as a kernel argument
struct TransposeTable {
  static constexpr int MAX = 64, TILE = 64;   // matrices per launch, tile edge
  int n = 0, total_tiles = 0;
  int64_t src_off[MAX], dst_off[MAX];
  int rows[MAX], cols[MAX], tile_begin[MAX + 1];
};
int launch_transpose_many(const float* params, bf16* tbase, const TransposeTable& tab, hipStream_t s);

// ---- k_layernorm.hip --------------------------------------------------------------------------------
// y = LN(x [+ branch]); with a branch (dtype y_dt) the sum is also written to x_out (fp32): the fused residual add
int launch_layernorm_fwd(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                         const float* beta, float eps, int64_t rows, int dim, int y_dt, void* y, float* mean, float* rstd,
                         hipStream_t s, const float* image_scale = nullptr, int rows_per_image = 0);
// Second stages of several two-stage column reductions, run by ONE launch (passed by value as a kernel argument): the
// backward pass queues the dgamma / dbeta reduction of each of its LayerNorms here instead of launching 27 small,
// latency-bound kernels between the big ones.
struct PartialsTable {
  static constexpr int MAX = 64;
  int n = 0;
  const float* partial[MAX];
  float *out0[MAX], *out1[MAX];
  int G[MAX], C[MAX], split[MAX], block_begin[MAX + 1];
};
int launch_sum_partials_many(const PartialsTable& tab, hipStream_t s);
// `defer` != null: the dgamma / dbeta second stage is appended to *defer (the caller keeps `partial` alive and launches
// launch_sum_partials_many later) instead of being launched here
int launch_layernorm_bwd(const void* dy, int dy_dt, const float* x, const int32_t* row_map, const float* gamma,
                         const float* mean, const float* rstd, int64_t rows, int dim, int accumulate, float* dx_io,
                         void* dx_copy, float* dgamma, float* dbeta, float* partial, hipStream_t s, PartialsTable* defer = nullptr,
                         const float* copy_scale = nullptr, int rows_per_image = 0);
constexpr int LN_BWD_MAX_BLOCKS = 1024;

// Compute units of the current device (256 on MI355X), queried once: the persistent GEMMs launch one workgroup per CU.
int num_cus();

// ---- GEMM family ------------------------------------------------------------------------------------
struct Epi {
  int mode = MAE_EPI_NONE;
  const float* bias = nullptr;
  const void* aux = nullptr;  // RESID: fp32 residual (M,N); DGELU: saved pre-activation (M,N) in out_dt
  void* out = nullptr;
  void* out2 = nullptr;       // GELU: activated output
  int out_dt = MAE_F32;
};
// out[M,N] = A[M,K] * W[N,K]^T
int launch_linear_fwd(const void* A, const void* W, int64_t M, int N, int K, int dt, const Epi& epi, hipStream_t s);
// dX[M,K] = dY[M,N] * W[N,K]   (epi.mode NONE or DGELU; bias unused)
int launch_linear_dgrad(const void* dY, const void* W, int64_t M, int N, int K, int dt, const Epi& epi, hipStream_t s);
// dW[N,K] (fp32, written) = dY[M,N]^T * A[M,K]; db[N] = colsum(dY) (may be null)
int64_t linear_wgrad_scratch_bytes(int64_t M, int N, int K);
int launch_linear_wgrad(const void* dY, const void* A, int64_t M, int N, int K, int dt, float* dW, float* db,
                        void* scratch, hipStream_t s);
int64_t linear_wgrad_pair_scratch_bytes(int64_t M, int N0, int K0, int N1, int K1);
int launch_linear_wgrad_pair(const void* dY0, const void* A0, int N0, int K0, float* dW0, float* db0, const void* dY1, const void* A1,
                             int N1, int K1, float* dW1, float* db1, int64_t M, int dt, void* scratch, hipStream_t s);

// ---- attention ------------------------------------------------------------------------------------------
int launch_attention_fwd(const void* qkv, int B, int T, int H, int hd, int dt, void* out, float* lse, hipStream_t s);
int launch_attention_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, int B, int T, int H,
                         int hd, int dt, void* d_qkv, hipStream_t s);
// Attention maps (k_attnmap.hip) from a block's qkv (B, T, 3, H, hd): per_head + b * per_head_stride + h * T + j = sum_t w[b,t] P_{b,h}[t,j]
// and / or mixed[b,j] = w[b,j] / 2 + sum_h per_head[b,h,j] / (2 H), one rollout step; fp32, fixed orders, no atomics.  Every limit
// (T <= attention_colsum_max_tokens, -1 for an unsupported hd / dtype) is checked before the launch.
int attention_colsum_max_tokens(int hd, int dt);
int launch_attention_colsum(const void* qkv, int dt, int B, int T, int H, int hd, const float* w, float* per_head, int64_t per_head_stride,
                            float* mixed, hipStream_t s);
// w (B, T) = row `row` of the identity in every image, or 1 / T everywhere for row < 0
int launch_attention_weight_fill(float* w, int B, int T, int row, hipStream_t s);

}  // namespace mae
