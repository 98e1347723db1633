/*
 * mae_hip.h -- C ABI of libmae_hip.so, the MI355X (gfx950) engine behind the reference's
 * MaskedAutoencoder boundary (reference: src/models/mae.py:12-94; step semantics
 * src/training/mae.py:40-83, scripts/training/pretrain_mae.py:116-126).
 *
 * The reference is pure Python and has no FFI of its own; the symbols below are what a
 * ctypes binding in the reference's src/models/mae.py would load.
 * Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch-ROCm caching allocator);
 *     the library borrows it for the duration of the call, allocates nothing on the device
 *     and keeps no pointer after the call returns;
 *   - every function enqueues work on `stream` (a hipStream_t passed as void*) and returns
 *     without synchronising; it is safe to capture into a hipGraph;
 *   - return value 0 = ok; non-zero = error, text via mae_last_error() (thread-local);
 *     no exception ever crosses this boundary;
 *   - "act dtype" selects the arithmetic of the branch tensors (LayerNorm outputs, q/k/v,
 *     MLP hidden, their gradients): MAE_F32 = exact fp32 path (parity), MAE_BF16 = bf16
 *     operands with fp32 accumulation on the MFMA units (throughput).  The residual stream,
 *     LayerNorm statistics, losses, gradients of parameters and optimizer state are fp32
 *     in both modes;
 *   - token indices are int64 on the API (as torch.argsort returns them) and int32 inside;
 *   - images are (batch, C, H, W) NCHW, either MAE_F32 (already normalised, what the reference's
 *     DataLoader yields after ToTensor + Normalize(.5,.5), src/data.py:15-24) or MAE_U8 (raw pixels
 *     as the STL-10 file stores them): with MAE_U8 the kernels that read pixels apply
 *     (u8/255 - 0.5)/0.5 themselves, bit-identical to the torch expression, and fetch every
 *     image byte once per kernel.
 */
#ifndef MAE_HIP_H
#define MAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAE_ABI_VERSION 4

enum { MAE_F32 = 0, MAE_BF16 = 1, MAE_U8 = 2 /* images only */ };

/* parameter flags (mae_engine_param_info) */
enum {
  MAE_PARAM_TRAINABLE = 1,   /* receives a gradient on the MAE path; clip + AdamW touch it     */
  MAE_PARAM_FROZEN    = 2,   /* requires_grad=False in the reference (sin-cos position tables)  */
  MAE_PARAM_UNUSED    = 4,   /* trainable in the reference but unreachable on this path:
                                encoder.mask_token (encode() is called with idx_mask=None,
                                src/models/mae.py:55) -> grad None -> skipped by AdamW/clip     */
  MAE_PARAM_MATRIX    = 8    /* 2-D GEMM weight (out, in): has a bf16 copy and a transposed copy */
};

/* Replaces the three ctor dicts of MaskedAutoencoder.__init__ (src/models/mae.py:15-52). */
typedef struct mae_config {
  int32_t image_size, patch_size, in_chans;
  int32_t embed_dim, depth, num_heads;
  int32_t decoder_embed_dim, decoder_depth, decoder_num_heads;
  int32_t mlp_ratio;      /* timm default 4 */
  int32_t act_dtype;      /* MAE_F32 | MAE_BF16 */
  int32_t pred_dim;       /* width of the prediction head: 0 = patch_size^2 * in_chans (MAE pixel targets);
                             embed_dim for the I-JEPA engine (latent targets), where the "decoder" is the predictor */
  int32_t norm_pix_loss;  /* != 0: the MAE loss regresses every masked patch standardised by its own mean and variance (see
                             MAE_NORM_PIX_EPS); needs pred_dim = 0.  0 = raw normalised pixels */
  int32_t reserved[3];
} mae_config_t;

/* Normalised-pixel targets (the MAE paper's norm_pix_loss), fixed definition.  For a patch x of P = p*p*C values in (py, px, c)
 * order, as mae_patchify_gather returns it (uint8 pixels after (u8/255 - 0.5)/0.5):
 *   mean = sum(x) / P;  var = sum((x - mean)^2) / (P - 1)  (unbiased, torch.var);  t = (x - mean) / sqrt(var + MAE_NORM_PIX_EPS).
 * Statistics are fp32 and two-pass (centred, then squared); a constant patch gives var == 0 and t == 0 exactly.  The
 * summation order depends on P alone: no atomics, a row is bit-identical from run to run, in any batch and from either
 * image dtype. */
#define MAE_NORM_PIX_EPS 1e-6

typedef struct mae_engine mae_engine_t;

const char* mae_last_error(void);
int         mae_abi_version(void);

/* ------------------------------------------------------------------------------------------
 * Engine: the whole path of MaskedAutoencoder.forward + MSE + backward + clip + AdamW.
 * ---------------------------------------------------------------------------------------- */
int  mae_engine_create(const mae_config_t* cfg, mae_engine_t** out);   /* src/models/mae.py:15-52 */
void mae_engine_destroy(mae_engine_t* e);

/* Parameter arena: one flat fp32 buffer.  Trainable-on-path tensors come first (so that clip and
 * AdamW run over one contiguous range [0, mae_engine_trainable_elems)), then frozen/unused ones.
 * Each tensor starts at a multiple of 64 elements; padding is zero and stays zero. */
int64_t mae_engine_num_params(const mae_engine_t* e);
int64_t mae_engine_arena_elems(const mae_engine_t* e);
int64_t mae_engine_trainable_elems(const mae_engine_t* e);
/* name: state_dict key, shape[4], flags: MAE_PARAM_*.  Order = state_dict order. */
int mae_engine_param_info(const mae_engine_t* e, int64_t index, const char** name, int64_t* offset,
                          int64_t* numel, int32_t* ndim, int64_t shape[4], int32_t* flags);

/* Workspace (saved activations + scratch) for `batch` images with `num_keep` visible tokens. */
int64_t mae_engine_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_keep);

/* Refresh the bf16 / transposed-bf16 operand copies of the GEMM weights from the fp32 arena.
 * Needed after the caller changed parameters behind the engine's back (load_state_dict, an
 * external optimizer).  mae_engine_optimizer_step does it itself.  No-op in MAE_F32 mode.
 * wcache: mae_engine_wcache_bytes() bytes. */
int64_t mae_engine_wcache_bytes(const mae_engine_t* e);
int mae_engine_refresh_weights(mae_engine_t* e, const float* params, void* wcache, void* stream);

/* lightly utils.random_token_mask with the noise draw made explicit (src/models/mae.py:79-83):
 * noise (batch, L) fp32 -> idx_keep (batch, num_keep), idx_mask (batch, L-num_keep), int64,
 * ascending noise, column 0 forced to -1 (class token always kept, always first), ties broken
 * by lower index (stable). */
int mae_mask_from_noise(const float* noise, int32_t batch, int32_t seq_len, int32_t num_keep,
                        int64_t* idx_keep, int64_t* idx_mask, void* stream);

/* MaskedAutoencoder.forward_encoder(images, idx_keep) (src/models/mae.py:54-55).
 * images (batch, C, H, W) NCHW in image_dtype (MAE_F32 | MAE_U8); idx_keep (batch, num_keep) int64 token ids in [0, L);
 * x_encoded (batch, num_keep, D) fp32.  Saves what backward needs in `workspace`. */
int mae_engine_forward_encoder(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                               int32_t image_dtype, const int64_t* idx_keep, int32_t batch, int32_t num_keep,
                               void* workspace, int64_t workspace_bytes, float* x_encoded, void* stream);

/* MaskedAutoencoder.forward_decoder(x_encoded, idx_keep, idx_mask) (src/models/mae.py:57-75).
 * x_encoded may be NULL = "use the encoder output already in workspace" (the fused forward).
 * x_pred (batch, L-num_keep... = num_mask, p*p*C) fp32. */
int mae_engine_forward_decoder(mae_engine_t* e, const float* params, const void* wcache, const float* x_encoded,
                               const int64_t* idx_keep, const int64_t* idx_mask, int32_t batch, int32_t num_keep,
                               int32_t num_mask, void* workspace, int64_t workspace_bytes, float* x_pred,
                               void* stream);

/* lightly utils.patchify + get_at_index(idx_mask-1) (src/models/mae.py:90-92):
 * target (batch, num_mask, p*p*C) fp32, per-patch order (py, px, c). */
int mae_patchify_gather(const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch,
                        int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float* target,
                        void* stream);

/* mae_patchify_gather with every row standardised (MAE_NORM_PIX_EPS above): target (batch, num_mask, p*p*C) fp32; mean / rstd
 * (batch, num_mask) fp32 = the row's mean and 1 / sqrt(var + eps), each may be NULL.  idx_mask entries are clamped like
 * mae_patchify_gather's (patch clamp(id - 1, 0, num_patches - 1)).  Limits, checked before the launch: image_size %
 * patch_size == 0, 2 <= p*p*C <= 10236 (four patches share the LDS); fp32 buffers 4-byte aligned.  Any patch size (not only
 * multiples of 4) and both image dtypes. */
int mae_patchify_gather_norm(const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch, int32_t in_chans,
                             int32_t image_size, int32_t patch_size, int32_t num_mask, float* target, float* mean /* may be NULL */,
                             float* rstd /* may be NULL */, void* stream);
/* The inverse: out = pred * sqrt(var + eps) + mean with the statistics of the ORIGINAL image's patch idx_mask[b][j] -- takes a
 * prediction made in normalised space back to pixel space.  pred, out (batch, num_mask, p*p*C) fp32; out may be pred itself
 * (a partial overlap is rejected).  Limits as mae_patchify_gather_norm. */
int mae_norm_pix_restore(const void* images, int32_t image_dtype, const float* pred, const int64_t* idx_mask, int32_t batch,
                         int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float* out, void* stream);

/* The augmentation step in front of the path: transforms.RandomResizedCrop(96, scale=(0.8, 1.0)) +
 * RandomHorizontalFlip() on the uint8 image, before ToTensor (src/data.py:15-20).  params (batch, 5)
 * int32 = (top, left, height, width, flip) per image, drawn by the caller (torchvision's get_params
 * rule, ssrl_vit_mae_jepa_amd/data.py); the box is resampled bilinearly to image_size x image_size
 * (pixel centres aligned, border clamp), rounded to uint8, columns mirrored when flip != 0.
 * images, out (batch, C, S, S) uint8, out != images. */
int mae_augment_crop_flip_u8(const uint8_t* images, const int32_t* params, int32_t batch, int32_t in_chans,
                             int32_t image_size, uint8_t* out, void* stream);

/* The same step to another size (additive in ABI v4): the box of every image resampled to out_size x out_size, so that a dataset
 * resident at one resolution feeds a model of another -- RandomResizedCrop(size) + RandomHorizontalFlip() for training,
 * Resize(size) for evaluation (src/data.py:15-34) -- in one pass.
 *   images : (batch, C, in_size, in_size), MAE_U8 raw pixels or MAE_F32 values;   out: (batch, C, out_size, out_size);
 *   params : (batch, 5) int32 = (top, left, height, width, flip) in source pixels; NULL = the whole image, not flipped.
 * Per axis (x shown; ox' = out_size - 1 - ox when flip != 0), with s = width / out_size and
 * c = left + width (2 ox' + 1) / (2 out_size) - 0.5 (the convention of mae_augment_crop_flip_u8):
 *   width <= out_size: c clamped to [0, in_size - 1]; taps floor(c), min(floor(c) + 1, in_size - 1), weights (1 - a, a);
 *   width >  out_size: the antialiasing triangle filter: taps j with |j - c| < s, those outside the image dropped, weight
 *                      1 - |j - c| / s divided by the sum of the kept weights.
 * The axes decide independently; the pixel is the separable weighted sum in fp32 (F.interpolate(mode="bilinear",
 * antialias=True, align_corners=False) for a whole-image box).  The border is the image edge, not the box edge.
 *   MAE_U8 -> MAE_U8 : rounded to nearest even and clamped to [0, 255];
 *   MAE_U8 -> MAE_F32: that byte through (v / 255 - 0.5) / 0.5, bit-identical to the engine's pixel kernels;
 *   MAE_F32 -> MAE_F32: the sum as it is;   MAE_F32 -> MAE_U8 is an error.
 * An output pixel whose centre falls on a source pixel copies it bit for bit (the identity box, a flip alone).
 * Errors before any launch: NULL images / out, a non-positive batch / in_chans / size, a size above 8192,
 * in_size > 8 * out_size (at most 17 taps an axis), an unknown dtype, out overlapping images, a float buffer or params not
 * 4-byte aligned.  The boxes are device data and are not checked: the kernel clamps top / left to [-in_size, 2 in_size],
 * height / width to [0, 2 in_size] and every tap index into the image, so no value reads outside the batch; the caller
 * validates 0 <= top, top + height <= in_size, height >= 1 (and the columns) if it wants the definition above. */
int mae_resize_crop_flip(const void* images, int32_t in_dtype, int32_t batch, int32_t in_chans, int32_t in_size,
                         const int32_t* params, int32_t out_size, int32_t out_dtype, void* out, void* stream);

/* torch.nn.MSELoss() (src/training/mae.py:40,48) over n elements, and its gradient w.r.t. pred
 * scaled by grad_scale: loss[0] = mean((pred-target)^2); d_pred = grad_scale*2*(pred-target)/n.
 * scratch: >= 4096 floats. */
int mae_mse_loss(const float* pred, const float* target, int64_t n, float grad_scale, float* loss,
                 float* d_pred /* may be NULL */, float* scratch, void* stream);

/* The loss of an engine created with norm_pix_loss, on caller buffers: mae_mse_loss between pred (batch, num_mask, p*p*C) fp32 and
 * the standardised patches idx_mask of images, which are never written to memory (n = batch * num_mask * p*p*C).
 * d_pred (may be NULL) in d_pred_dtype MAE_F32 | MAE_BF16; the target carries no gradient.  scratch: >= 4096 floats.
 * Limits as mae_patchify_gather_norm; d_pred 4-byte (fp32) / 2-byte (bf16) aligned. */
int mae_mse_loss_norm_pix(const float* pred, const void* images, int32_t image_dtype, const int64_t* idx_mask, int32_t batch,
                          int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask, float grad_scale, float* loss,
                          void* d_pred /* may be NULL */, int32_t d_pred_dtype, float* scratch, void* stream);

/* Backward of forward_decoder(forward_encoder(.)) given d_pred (batch, num_mask, P) fp32.
 * Writes (not accumulates) every trainable gradient into grads[0 .. trainable_elems); summing the gradients of several
 * micro-batches is the caller's sweep with mae_engine_grad_accumulate (below).
 * Requires the workspace of the matching forward calls.  d_x_encoded_extra: optional extra
 * gradient (batch, num_keep, D) fp32 added at the encoder output (NULL on the MAE path): a second consumer of
 * x_encoded, e.g. a probe head trained next to the reconstruction loss. */
int mae_engine_backward(mae_engine_t* e, const float* params, const void* wcache, const float* d_pred,
                        const float* d_x_encoded_extra, int32_t batch, int32_t num_keep, int32_t num_mask,
                        void* workspace, int64_t workspace_bytes, float* grads, void* stream);

/* The two halves of mae_engine_backward, for callers that hold forward_encoder and forward_decoder as separate autograd
 * nodes (the reference's fine-tuning hands encoder.vit to a classifier: scripts/training/train_mae.py:143,
 * src/models/classifier.py:47-57).
 * _decoder: d_pred -> every decoder gradient (arena range [mae_engine_encoder_grad_elems, trainable_elems)) and, when
 *           d_x_encoded is not NULL, the gradient w.r.t. forward_decoder's x_encoded input (batch, num_keep, D) fp32.
 * _encoder: d_x_encoded (batch, num_keep, D) fp32 -> every encoder gradient (arena range [0, encoder_grad_elems)).
 * Each writes only its own range of `grads` and needs the workspace of the matching forward call. */
int64_t mae_engine_encoder_grad_elems(const mae_engine_t* e);
int mae_engine_backward_decoder(mae_engine_t* e, const float* params, const void* wcache, const float* d_pred,
                                int32_t batch, int32_t num_keep, int32_t num_mask, void* workspace,
                                int64_t workspace_bytes, float* grads, float* d_x_encoded, void* stream);
int mae_engine_backward_encoder(mae_engine_t* e, const float* params, const void* wcache, const float* d_x_encoded,
                                int32_t batch, int32_t num_keep, void* workspace, int64_t workspace_bytes,
                                float* grads, void* stream);

/* decoder.decode(x) (lightly MAEDecoderTIMM, called at src/models/mae.py:71): x (batch, L, Dd) fp32 ->
 * decoder_norm(blocks(x + decoder_pos_embed)) for EVERY row, (batch, L, Dd) fp32.  Inference only (saves nothing).
 * decoder.embed / decoder.predict (src/models/mae.py:59,73) are plain Linears: mae_linear_fwd. */
int mae_engine_decoder_decode(mae_engine_t* e, const float* params, const void* wcache, const float* x, int32_t batch,
                              void* workspace, int64_t workspace_bytes, float* out, void* stream);

/* One fused pass: zero_grad + mask + forward + MSE + backward (training_step + loss.backward(),
 * src/training/mae.py:45-50).  noise (batch, L) fp32.  loss_out[0] = batch-mean MSE (against the standardised patches when the
 * engine was created with norm_pix_loss: mae_mse_loss_norm_pix; nothing else of the step changes).
 * grad_scale multiplies the loss gradient (1/world_size for data-parallel sum-all-reduce).
 * idx_keep_out/idx_mask_out: optional int64 outputs (may be NULL). */
int mae_engine_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                              int32_t image_dtype, const float* noise, int32_t batch, int32_t num_keep, float grad_scale,
                              void* workspace, int64_t workspace_bytes, float* grads, float* loss_out,
                              int64_t* idx_keep_out, int64_t* idx_mask_out, void* stream);

/* Data-parallel overlap (no counterpart in the reference, which runs devices=1, scripts/training/pretrain_mae.py:118).
 * The backward pass finishes the gradient arena from its END: the decoder's tensors first, then encoder block depth-1,
 * ..., block 0, patch projection and class token last.  mae_engine_grad_ready_points reports those points in the order
 * they are reached: reaching point j means grads[offsets[j] .. trainable_elems) is final.  Returns the number of
 * points (encoder depth + 1; the last one has offset 0); fills at most max_points offsets (offsets may be NULL). */
int32_t mae_engine_grad_ready_points(const mae_engine_t* e, int64_t* offsets, int32_t max_points);
/* mae_engine_loss_and_grads that also records ready_events[j] (a hipEvent_t passed as void*; NULL = skip the point) on
 * `stream` when point j is reached, so that the caller can start the all-reduce of that arena range on another stream
 * while the rest of the backward pass still runs.  num_ready must equal mae_engine_grad_ready_points(). Results are
 * bit-identical to mae_engine_loss_and_grads. */
int mae_engine_loss_and_grads_phased(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                                     int32_t image_dtype, const float* noise, int32_t batch, int32_t num_keep, float grad_scale,
                                     void* workspace, int64_t workspace_bytes, float* grads, float* loss_out,
                                     int64_t* idx_keep_out, int64_t* idx_mask_out, void* const* ready_events,
                                     int32_t num_ready, void* stream);

/* clip_grad_norm_(max_norm, L2) (scripts/training/pretrain_mae.py:124-125) followed by
 * torch.optim.AdamW single-group step (src/training/mae.py:59-65) over the trainable range,
 * then the operand-copy refresh.  step is 1-based.  stats_out[0] = total grad norm (pre-clip),
 * stats_out[1] = clip coefficient.  exp_avg / exp_avg_sq: trainable_elems floats each.
 * scratch: >= 4096 floats. */
int mae_engine_optimizer_step(mae_engine_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                              void* wcache, float lr, float beta1, float beta2, float eps, float weight_decay,
                              float max_norm, int64_t step, float* stats_out, float* scratch, void* stream);

/* ------------------------------------------------------------------------------------------
 * I-JEPA step (BASELINE.json configs[2] and [4]).  The reference has NO I-JEPA code ("JEPA" only in README.md:1,9 and
 * pyproject.toml:2), so nothing here replaces a reference function: the specification is DESIGN.md section "I-JEPA"
 * (I-JEPA paper), built from the same ViT pieces.  The engine must be created with pred_dim = embed_dim; its
 * "decoder" tensors are the predictor.  Token ids are patch tokens 1 .. N (0, the class token, is not used).
 *   idx_context (batch, num_context) int64: context tokens of every image (same count for all: truncated to the minimum);
 *   idx_target  (batch, num_blocks, block_tokens) int64: the target blocks;
 *   target_params / target_wcache: the EMA target encoder, an arena of the same layout (only the encoder part is read);
 *   loss over all batch * num_blocks * block_tokens * D elements between predictor output and
 *   layer_norm(target_encoder(images))[targets] (no affine, eps 1e-5); loss_kind MAE_LOSS_MSE | MAE_LOSS_SMOOTH_L1.
 * grads == NULL: compute the targets only.  h_out / pred_out: optional fp32 copies (batch*num_blocks*block_tokens, D).
 * ready_events: as mae_engine_loss_and_grads_phased (may be NULL, then num_ready is ignored). */
enum { MAE_LOSS_MSE = 0, MAE_LOSS_SMOOTH_L1 = 1 };
int64_t mae_engine_jepa_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_context, int32_t num_blocks,
                                        int32_t block_tokens);
int mae_engine_jepa_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const float* target_params,
                                   const void* target_wcache, const void* images, int32_t image_dtype,
                                   const int64_t* idx_context, const int64_t* idx_target, int32_t batch,
                                   int32_t num_context, int32_t num_blocks, int32_t block_tokens, int32_t loss_kind,
                                   float grad_scale, void* workspace, int64_t workspace_bytes, float* grads,
                                   float* loss_out, float* h_out, float* pred_out, void* const* ready_events,
                                   int32_t num_ready, void* stream);
/* The optimizer on a SHARD of the parameter arena (ABI v4; data-parallel ranks that each own 1 / world of the trainable range, the
 * reduce-scatter -> shard sum of squares -> scalar all-reduce -> AdamW on the shard -> all-gather scheme).  The reference runs one
 * replicated clip_grad_norm_ + AdamW (scripts/training/pretrain_mae.py:124-125, src/training/mae.py:59-65); these three calls are that
 * step cut at the two points where ranks have to talk.  lo, count: float offsets into the arenas, multiples of 4, inside
 * [0, mae_engine_trainable_elems).
 *   mae_engine_grad_sumsq_range: sumsq_out[0] = sum of grads[lo .. lo+count)^2 (count may be 0)
 *   mae_engine_clip_from_sumsq : stats_out = {sqrt(sumsq[0]), min(1, max_norm / (sqrt(sumsq[0]) + 1e-6))} -- after the ranks' sums were added
 *   mae_engine_adamw_range     : AdamW on [lo, lo+count) with gradients scaled by stats[1]; writes the bf16 operand copy of that range only.
 *                                Call mae_engine_refresh_weights once the shards have been gathered. */
int mae_engine_grad_sumsq_range(mae_engine_t* e, const float* grads, int64_t lo, int64_t count, float* sumsq_out, float* scratch,
                                void* stream);
int mae_engine_clip_from_sumsq(mae_engine_t* e, const float* sumsq, float max_norm, float* stats_out, void* stream);
int mae_engine_adamw_range(mae_engine_t* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* wcache,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* stats,
                           int64_t lo, int64_t count, void* stream);

/* Gradient accumulation over micro-batches (additive in ABI v4; Lightning's Trainer(accumulate_grad_batches=A), which the reference's
 * scripts leave at 1).  Every *_loss_and_grads call WRITES its gradients, so a window of A micro-batches that feeds one optimizer
 * step keeps a second buffer of the same layout (the stash) and sums into it between the calls:
 *   dst[lo .. lo+count) = (overwrite ? 0 : dst[lo .. lo+count)) + src[lo .. lo+count)
 * with exactly one fp32 add per element and no atomics (deterministic).  With overwrite the source is copied bit for bit and dst
 * is not read.  lo, count: float offsets as in mae_engine_adamw_range, multiples of 4, but into the caller's own buffers (no engine
 * range bounds them: a gradient arena with its loss slot, a head gradient, ...); count == 0 succeeds without a launch; dst + lo and
 * src + lo must be 16-byte aligned and the two ranges must not overlap.  All of that is checked before any launch.  One streaming
 * sweep of 12 bytes per element (8 with overwrite) on a grid of at most MAE_GRAD_ACC_BLOCKS blocks of 256 threads, 4 floats a thread.
 * The optimizer calls are untouched: an accumulated step and a plain step share them. */
enum { MAE_GRAD_ACC_BLOCKS = 2048 };
int mae_engine_grad_accumulate(mae_engine_t* e, float* dst, const float* src, int64_t lo, int64_t count, int32_t overwrite,
                               void* stream);

/* Downstream classifier (additive in ABI v4): ViTClassifier + ViTClassifierTrainModule of the reference
 * (src/models/classifier.py:47-57, src/training/classifier.py:75-171), i.e. the encoder over EVERY token (timm
 * forward_features, scripts/training/train_mae.py:143), pooled = feats[:, 0] (MAE_POOL_CLS) or feats.mean(dim=1) over all
 * L = 1 + num_patches rows (MAE_POOL_MEAN), logits = pooled @ W.T + b, loss = F.cross_entropy(logits, labels) (batch mean),
 * correct = sum(logits.argmax(1) == labels) (first index among equal maxima).
 *   head: the head's own fp32 buffer, W (num_classes, embed_dim) row-major then b (num_classes) -- not part of the arena;
 *   labels: (batch) int64 in [0, num_classes); a label outside that range is never read through: that batch's loss is NaN
 *           (and so are the gradients of its row);
 *   num_classes in [2, 128]; logits (batch, num_classes) fp32, loss_out (1) fp32, correct_out (1) int32 -- each may be NULL.
 *   workspace: mae_engine_classifier_workspace_bytes(batch, num_classes) bytes (it is also a valid workspace of
 *              mae_engine_workspace_bytes(batch, L) layout: the classifier overwrites the saved activations of any forward).
 * mae_engine_classifier_forward: inference (no activation is saved for a backward); labels may be NULL when loss_out and
 *   correct_out are.
 * mae_engine_classifier_loss_and_grads: forward + loss + backward over the trainable set
 *   train_blocks = -1 : encoder frozen (linear probe, freeze_encoder()): only head_grads is written;
 *   train_blocks = n  : blocks[depth-n:] and the final norm (unfreeze_last_layers(n), :139-171): their gradients land in
 *                       `grads` (the arena-shaped trainable-range buffer) at their usual offsets; nothing else of `grads` is
 *                       written and no block below depth-n runs;
 *   train_embed = 1   : n = depth only -- also cls_token, patch_embed.proj.* (in `grads`) and pos_embed, whose gradient
 *                       goes to pos_grad (L * embed_dim floats, it lies outside the trainable range) (unfreeze_encoder(), :134).
 *   head_grads: dW then db, same layout as head.  grad_scale multiplies every gradient (not the loss). */
enum { MAE_POOL_CLS = 0, MAE_POOL_MEAN = 1, MAE_POOL_MEAN_PATCHES = 2 /* features and the _ex classifier calls; the three calls below reject it */,
       MAE_POOL_CLS_MEAN_PATCHES = 3 /* [class row | patch mean], 2 * dim wide: mae_engine_extract_layer_features and mae_features_tap only */ };
int64_t mae_engine_classifier_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_classes);
int mae_engine_classifier_forward(mae_engine_t* e, const float* params, const void* wcache, const float* head, const void* images,
                                  int32_t image_dtype, const int64_t* labels, int32_t batch, int32_t pool, int32_t num_classes,
                                  void* workspace, int64_t workspace_bytes, float* logits, float* loss_out, int32_t* correct_out,
                                  void* stream);
int mae_engine_classifier_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                         const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                         int32_t pool, int32_t num_classes, int32_t train_blocks, int32_t train_embed,
                                         float grad_scale, void* workspace, int64_t workspace_bytes, float* grads,
                                         float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                         int32_t* correct_out, void* stream);
/* The classifier on a sequence with or without the class token, and the patch-row mean (additive in ABI v4).  Arguments as
 * the three calls above, plus with_cls in front of pool:
 *   with_cls = 1: [cls | patch 1..N], L = N + 1 rows per image (the calls above);
 *   with_cls = 0: patch tokens 1..N only -- the sequence an I-JEPA encoder was trained on.  Row j carries pos_embed[j + 1];
 *                 cls_token and pos_embed[0] take no part in the forward.
 *   pool: MAE_POOL_CLS          row 0; with_cls = 1 only (with_cls = 0 is an error before any launch: no class token);
 *         MAE_POOL_MEAN         mean over every row of the sequence (L with the class token, N without);
 *         MAE_POOL_MEAN_PATCHES mean over the patch rows: rows 1..L-1 with the class token (timm global_pool = "avg", the
 *                               MAE fine-tuning recipe), every row without (the same as MAE_POOL_MEAN, bit for bit).
 *   Backward: the feature gradient is d_pooled / rows_pooled on the pooled rows; with MAE_POOL_MEAN_PATCHES the class-token
 *   row gets exact zeros and the final LayerNorm backward still runs over all rows.  With with_cls = 0 and train_embed = 1,
 *   pos_grad (still L * embed_dim floats) holds the sums in rows 1..N and exact zeros in row 0, and the cls_token slot of
 *   `grads` is written as exact zeros: an optimizer with weight decay must leave those two tensors out.
 *   Deterministic: fixed summation orders, no atomics.  embed_dim a multiple of 4, at most 1024.
 *   with_cls = 1 and MAE_POOL_CLS / MAE_POOL_MEAN run exactly the launches of the calls above.
 *   workspace: mae_engine_classifier_workspace_bytes_ex(batch, num_classes, with_cls) bytes. */
int64_t mae_engine_classifier_workspace_bytes_ex(const mae_engine_t* e, int32_t batch, int32_t num_classes, int32_t with_cls);
int mae_engine_classifier_forward_ex(mae_engine_t* e, const float* params, const void* wcache, const float* head, const void* images,
                                     int32_t image_dtype, const int64_t* labels, int32_t batch, int32_t with_cls, int32_t pool,
                                     int32_t num_classes, void* workspace, int64_t workspace_bytes, float* logits, float* loss_out,
                                     int32_t* correct_out, void* stream);
int mae_engine_classifier_loss_and_grads_ex(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                            const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                            int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                            int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                            float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                            int32_t* correct_out, void* stream);
/* Soft targets for fine-tuning (additive in ABI v4): mae_engine_classifier_loss_and_grads_ex with the loss of the MAE / DeiT
 * fine-tuning recipe -- mixup / CutMix label pairs and label smoothing.  The target of row b is
 *   t[b][c] = eps / C + (1 - eps) * (lam[b] * [c == labels[b]] + (1 - lam[b]) * [c == labels_b[b]]),   C = num_classes,
 * loss = mean_b (lse_b - sum_c t[b][c] * logit[b][c]) and d_logits = (softmax - t) * grad_scale / batch, rounded where the hard
 * loss rounds it; this is lam * CE(labels, label_smoothing = eps) + (1 - lam) * CE(labels_b, label_smoothing = eps) of torch.
 *   labels_b: (batch) int64 on the device, NULL = labels;  lam: (batch) fp32 on the device, NULL = 1;
 *   label_smoothing = eps in [0, 1) (else an error before any launch).
 *   correct_out still counts argmax == labels[b] (the first label of a pair).  A label outside [0, num_classes) in labels OR
 *   labels_b is never used as an index: that row's loss and gradients are NaN.  Deterministic as the calls above.
 * With labels_b == NULL, lam == NULL and label_smoothing == 0 the call runs exactly the launches of
 * mae_engine_classifier_loss_and_grads_ex (same bits).  Evaluation stays hard-label: there is no soft forward call. */
int mae_engine_classifier_loss_and_grads_soft(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                              const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                              int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                              int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                              float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                              int32_t* correct_out, const int64_t* labels_b, const float* lam, float label_smoothing,
                                              void* stream);
/* Stochastic depth / drop path for fine-tuning (additive in ABI v4; timm DropPath, scale_by_keep): the _soft call above plus
 * branch_scale, a caller-owned device table (2 * depth, batch) fp32.  Row 2i holds the per-image scale of the attention branch of
 * encoder block i, row 2i + 1 that of its MLP branch:
 *   x_mid = x_in + branch_scale[2i][b] * attn(LN1(x_in)),   x_out = x_mid + branch_scale[2i + 1][b] * mlp(LN2(x_mid)).
 * The engine does not draw: any finite values are taken (0 = dropped, 1 / (1 - p) = kept at rate p).  The product is formed in fp32
 * inside the LayerNorm kernel that does the residual add, after the branch was rounded to the activation dtype; a scale of exactly 0
 * does not read the branch.  The backward multiplies the activation-dtype copy of the residual gradient that each branch reads by the
 * same scale (one fp32 product, then the rounding of the copy).  No extra launch, buffer or pass over memory.
 *   branch_scale == NULL: exactly the launches of mae_engine_classifier_loss_and_grads_soft (same bits).
 *   branch_scale != NULL with train_blocks = -1 is refused before any launch: the probe's encoder is in inference and never drops. */
int mae_engine_classifier_loss_and_grads_sd(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                            const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                            int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                            int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                            float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                            int32_t* correct_out, const int64_t* labels_b, const float* lam, float label_smoothing,
                                            const float* branch_scale, void* stream);
/* Batch mixing in front of that loss (additive in ABI v4; timm's Mixup in `batch` mode): image b is mixed with image
 * partner[b] of the same batch into out (batch, C, S, S), which may not overlap images (checked).
 *   images : (batch, C, S, S), MAE_U8 raw pixels or MAE_F32 normalised values; n() below is the engine's uint8 normalisation
 *            (x / 255 - 0.5) / 0.5 for MAE_U8 (bit-identical to what its pixel kernels produce) and the identity for MAE_F32;
 *   partner: (batch) int32; a value outside [0, batch) is never used as an index -- that image is its own partner;
 *   lam    : (batch) fp32;   box: (batch, 4) int32 (y0, y1, x0, x1), half-open, clamped to [0, S] by the kernel; may be empty.
 *   out_dtype = MAE_F32: inside the box n(partner pixel); outside it lam * n(own) + (1 - lam) * n(partner) in fp32 (1 - lam, one
 *                        product and the sum round; lam == 1 copies n(own) bit for bit).
 *   out_dtype = MAE_U8 : pure CutMix on MAE_U8 images (MAE_F32 images are an error): the partner's byte inside the box, the own
 *                        byte outside; lam is not read (may be NULL).  The batch stays 1 byte per pixel for the engine.
 * Any C >= 1 and 1 <= S <= 16384.  A thread moves V pixels, 16 bytes of output where the row length allows: V = 16 for MAE_U8
 * output with S % 16 == 0, else V = 4 when S % 4 == 0, else V = 1.  Limits, checked before the launch: batch * C * S * S / V <= 2^31 - 256;
 * MAE_U8 buffers V-byte aligned and MAE_F32 buffers 4 V-byte aligned (fp32 output at S = 96: images 4-byte if MAE_U8, 16-byte
 * if MAE_F32, out 16-byte; uint8 output at S = 96: both 16-byte); partner / lam / box 4-byte. */
int mae_mix_batch(const void* images, int32_t image_dtype, const int32_t* partner, const float* lam, const int32_t* box,
                  int32_t batch, int32_t in_chans, int32_t image_size, int32_t out_dtype, void* out, void* stream);

/* Per-image augmentation in front of the mixing (additive in ABI v4): RandomResizedCrop + flip, RandAugment and random erasing
 * of the MAE / BEiT / DeiT fine-tuning recipe on uint8 images, with the semantics of the PIL calls timm makes, per element.
 * One workgroup per image; the image stays in LDS through the whole chain (two buffers: op k + 1 reads the rounded uint8 result
 * of op k), so 2 * C * S * S + 3200 bytes must fit 160 KiB: S <= 160 at C = 3, else an error before the launch.
 *   images  : (batch, C, S, S) uint8;   out: (batch, C, S, S) in out_dtype, may neither be nor overlap images (checked);
 *   op_codes: (batch, num_ops, 2) int32: the op id and its integer argument;   num_ops in 0..8, ops applied in slot order;
 *   op_args : (batch, num_ops, 6) fp64: the blend factor in [0], or the affine matrix;
 *   erase   : (batch, 5) int32 (y0, y1, x0, x1, seed), half-open, clamped to [0, S] by the kernel, empty / inverted = nothing
 *             erased; NULL = none.
 * Ops (an id outside the list is NONE; an id is never used as an index):
 *   INVERT 255 - v;  SOLARIZE(t) v < t ? v : 255 - v;  SOLARIZE_ADD(a) v < 128 ? clamp(v + a, 0, 255) : v;
 *   POSTERIZE(bits) v & ~(2^(8 - bits) - 1) (bits >= 8 identity, bits <= 0 black);
 *   AUTOCONTRAST / EQUALIZE: ImageOps.autocontrast(cutoff 0) / ImageOps.equalize, per channel;
 *   COLOR / CONTRAST / BRIGHTNESS / SHARPNESS(f): ImageEnhance, Image.blend(degenerate, image, f) in fp32;
 *   AFFINE(m; integer argument = mode | fill << 8, fill = 0xRRGGBB, a one-channel image takes its low byte):
 *     Image.transform(AFFINE, m, resample, fillcolor) in fp64: mode 0 bilinear and 1 bicubic as PIL rounds them (truncation),
 *     2 / 3 the same filters rounded to nearest.  The random-resized crop is the map (w / S, 0, left, 0, h / S, top) of slot 0,
 *     (-w / S, 0, left + w, 0, h / S, top) when flipped; the identity box returns the image bit for bit.
 * Every op but AFFINE needs in_chans == 3: with another in_chans, num_ops > 0 is an error unless out_dtype carries
 * MAE_AUG_GEOMETRIC, the caller's statement that every id is AFFINE or NONE (the kernel then skips any other id).
 *   out_dtype = MAE_U8 : the bytes; erase is ignored (normal noise has no byte form).
 *   out_dtype = MAE_F32: (v / 255 - 0.5) / 0.5, bit-identical to the engine's pixel kernels; element e = (c S + y) S + x inside
 *     the erase box is N(0, 1) noise (timm RandomErasing, `pixel` mode): with fmix32 murmur3's finaliser and
 *     mix(s, i) = fmix32(fmix32(i + 0x9E3779B9) ^ s): u1 = ((mix(seed, 2e) >> 8) + 1) 2^-24, u2 = (mix(seed, 2e + 1) >> 8) 2^-24,
 *     n = sqrtf(-2 logf(u1)) cosf(2 pi u2).
 * op_codes / erase 4-byte, op_args 8-byte, an fp32 out 4-byte aligned. */
enum { MAE_AUG_NONE = 0, MAE_AUG_AUTOCONTRAST, MAE_AUG_EQUALIZE, MAE_AUG_INVERT, MAE_AUG_POSTERIZE, MAE_AUG_SOLARIZE,
       MAE_AUG_SOLARIZE_ADD, MAE_AUG_COLOR, MAE_AUG_CONTRAST, MAE_AUG_BRIGHTNESS, MAE_AUG_SHARPNESS, MAE_AUG_AFFINE };
enum { MAE_AUG_GEOMETRIC = 0x100 /* or-ed into out_dtype */ };
int mae_augment_ops_u8(const uint8_t* images, int32_t batch, int32_t in_chans, int32_t image_size, const int32_t* op_codes,
                       const double* op_args, int32_t num_ops, const int32_t* erase, int32_t out_dtype, void* out, void* stream);

/* The classifier's optimizer (Lightning gradient_clip_val = 1.0 + one-group torch AdamW over the requires_grad tensors,
 * scripts/training/train_mae.py:213, src/training/classifier.py:106-108) over buffers that are not the arena's trainable range:
 *   mae_engine_grad_sumsq_buffer       : sumsq_io[0] = (accumulate ? sumsq_io[0] : 0) + sum of grads[0 .. count)^2
 *                                        (sumsq_io holds 2 floats; [1] is a temporary); count a multiple of 4;
 *   mae_engine_adamw_buffer            : the AdamW of mae_engine_adamw_range (same device code, gradients scaled by stats[1])
 *                                        on a plain buffer (the head, pos_embed); count a multiple of 4;
 *   mae_engine_refresh_transposed_range: the transposed bf16 operand copies of the matrices inside [lo, lo+count) of the
 *                                        arena (mae_engine_adamw_range already wrote the straight copies of that range). */
int mae_engine_grad_sumsq_buffer(mae_engine_t* e, const float* grads, int64_t count, int32_t accumulate, float* sumsq_io,
                                 float* scratch, void* stream);
int mae_engine_adamw_buffer(mae_engine_t* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count,
                            float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* stats,
                            void* stream);
int mae_engine_refresh_transposed_range(mae_engine_t* e, const float* params, void* wcache, int64_t lo, int64_t count, void* stream);

/* Frozen-encoder features (additive in ABI v4; scripts/evaluation/visualize_representation.py:87-108 of the reference):
 * the encoder forward over every image, nothing saved for a backward, then ONE fused step that does the last residual add,
 * the final LayerNorm (encoder.vit.norm, eps 1e-6) in fp32, the pool and the optional normalisation, writing only
 * feats (batch, embed_dim) fp32.
 *   with_cls = 1: the sequence is [cls | patch 1..N] (timm forward_features, the classifier's sequence);
 *   with_cls = 0: patch tokens 1..N only (what the I-JEPA encoders see);
 *   params / wcache: any arena of the engine's layout (the I-JEPA EMA target arena included);
 *   pool: MAE_POOL_CLS (row 0; with_cls = 1 only), MAE_POOL_MEAN (mean over every row of the sequence, the classifier's
 *         mean), MAE_POOL_MEAN_PATCHES (mean over the patch rows: out[:, 1:].mean(1) with cls, every row without);
 *   normalize: MAE_FEAT_NONE, or MAE_FEAT_L2 = f / (||f||_2 + 1e-8).
 * embed_dim must be a multiple of 4 and at most 1024 (else both calls fail: -1 / an error, before any launch).
 * Deterministic (fixed summation orders, no atomics).  workspace: mae_engine_features_workspace_bytes(batch, with_cls)
 * bytes, 256-byte aligned; it overwrites the saved activations of any earlier forward that used the same buffer. */
enum { MAE_FEAT_NONE = 0, MAE_FEAT_L2 = 1 };
int64_t mae_engine_features_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls);
int mae_engine_extract_features(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                int32_t batch, int32_t with_cls, int32_t pool, int32_t normalize, void* workspace,
                                int64_t workspace_bytes, float* feats, void* stream);

/* Features after any encoder block (additive in ABI v4): ONE forward pass, and after every block layers[i] the fused step of
 * mae_engine_extract_features on the residual stream x_mid + mlp branch of that block, through the encoder's own final LayerNorm
 * (encoder.vit.norm, eps 1e-6: DINO's get_intermediate_layers, the I-JEPA last-n-layers probe), written to feats[:, i, :].
 *   layers: HOST array of num_layers 0-based block indices, strictly ascending, each in [0, depth); 1 <= num_layers <= depth.
 *           The forward stops after block layers[num_layers - 1].  Block depth - 1 gives mae_engine_extract_features' bits.
 *   pool: the three pools above (W = embed_dim), or MAE_POOL_CLS_MEAN_PATCHES (with_cls = 1 only): W = 2 embed_dim,
 *         feats[b][i] = [class row | mean over the patch rows], equal bit for bit to MAE_POOL_CLS and MAE_POOL_MEAN_PATCHES.
 *   normalize: MAE_FEAT_L2 normalises every embed_dim-wide slice (layer, and half of pool 3) on its own.
 *   feats: (batch, num_layers, W) fp32, 16-byte aligned.
 * Same limits, workspace (mae_engine_features_workspace_bytes) and determinism as the call above; every refusal comes before
 * any launch. */
int mae_engine_extract_layer_features(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                      int32_t batch, int32_t with_cls, int32_t pool, int32_t normalize, const int32_t* layers,
                                      int32_t num_layers, void* workspace, int64_t workspace_bytes, float* feats, void* stream);

/* Frozen-encoder tokens (additive in ABI v4): mae_engine_extract_features without the pool.  The encoder forward with nothing saved, the last
 * residual add and the final LayerNorm in fp32 (the step of the fused add + LayerNorm kernel, a bf16 branch widened first), written as
 * tokens (batch, T_out, embed_dim) fp32 in the sequence's order.
 *   with_cls as above: T = N + 1 rows [cls | patches], or the N patch rows;
 *   drop_cls = 1 (with_cls = 1 only): the class row is left out, T_out = N; else T_out = T.
 * Same limits, workspace rules and determinism; the workspace query returns what the features call asks for. */
int64_t mae_engine_tokens_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls);
int mae_engine_extract_tokens(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                              int32_t batch, int32_t with_cls, int32_t drop_cls, void* workspace, int64_t workspace_bytes,
                              float* tokens, void* stream);

/* Attention maps of the frozen encoder (additive in ABI v4): ONE forward pass that stops after block
 * layers[num_layers - 1], then mae_attention_colsum (below) over the blocks' saved qkv.  P_l,h = the attention probabilities of
 * head h of block l, (T, T), rows = queries.
 *   query: MAE_ATTN_QUERY_CLS (with_cls = 1 only): the start weight w is the class row e_0, a map is the class token's attention row
 *          (DINO's maps); MAE_ATTN_QUERY_MEAN: w = 1 / T in every column, a map is the mean attention each token receives.
 *   layers: HOST array as for mae_engine_extract_layer_features: strictly ascending, each in [0, depth); 1 <= num_layers <= depth.
 *   maps:    (batch, num_layers, H, T) fp32 or NULL: maps[b][i][h][j] = sum_t w[t] P_layers[i],h[t][j]; every (b, i, h) row sums to 1.
 *   rollout: (batch, T) fp32 or NULL (not both): row w A_top ... A_0 of attention rollout, A_l = (mean_h P_l,h + I) / 2,
 *            top = layers[num_layers - 1], down to block 0 whatever else layers names; computed as a chain of vector-matrix steps.
 * T = N + with_cls must not exceed mae_attention_colsum_max_tokens(head_dim, act dtype); head_dim and the head count within that
 * call's limits.  maps and rollout 16-byte aligned.  Workspace: mae_engine_attention_workspace_bytes = the features workspace.
 * Every refusal comes before any launch; results are bit-identical from run to run and an image's do not depend on its batch. */
enum { MAE_ATTN_QUERY_CLS = 0, MAE_ATTN_QUERY_MEAN = 1 };
int64_t mae_engine_attention_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls);
int mae_engine_extract_attention(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                 int32_t batch, int32_t with_cls, int32_t query, const int32_t* layers, int32_t num_layers, float* maps,
                                 float* rollout, void* workspace, int64_t workspace_bytes, void* stream);

/* MAE reconstruction (additive in ABI v4; scripts/evaluation/visualize_reconstruction.py of the reference, MAEReconstructor):
 * the inverse of mae_patchify_gather, fused with the whole-image error sums.  One pass over the OUTPUT pixels produces up to
 * three results from images (batch, C, S, S) in image_dtype (MAE_F32 normalised | MAE_U8 raw pixels, normalised in the read),
 * pred (batch, num_mask, p*p*C) fp32 in the per-patch order (py, px, c) of x_pred / mae_patchify_gather, and idx_mask
 * (batch, num_mask) int64 token ids:
 *   recon  (batch, C, S, S): the normalised image with every patch n = idx_mask[b][j] - 1 replaced by pred[b][j]
 *                            (_reconstruct_full_images, :198-234: patchify -> set_at_index -> unpatchify);
 *   masked (batch, C, S, S): the normalised image with those patches set to `fill` (_create_masked_images, :170-190; the
 *                            reference fills with 0.5, :185);
 *   stats  (batch, 2) fp32 : per image sum (recon - orig)^2 and sum |recon - orig| -- the numerators of nn.MSELoss() /
 *                            nn.L1Loss()(original, reconstructed) (:324-334).  The sums run over the replaced pixels (a visible
 *                            pixel contributes exactly 0), accumulate in fp32 in a fixed order that depends on the image shape
 *                            alone (no atomics: bit-identical from run to run and for any batch the image is part of).
 * Each of recon / masked / stats may be NULL (not all three).  recon and masked are written in out_dtype: MAE_F32 = normalised
 * values (visible pixels bit-identical to the normalised input, replaced ones bit-identical copies of pred); MAE_U8 = display
 * pixels round_half_even(clamp(v * 0.5 + 0.5, 0, 1) * 255) (_tensor_to_image, :311-322, then mul(255).round()), bit-identical
 * to the torch fp32 expression.  Every output byte is written exactly once; recon and masked may overlap neither images, pred nor each other (checked, partial
 * overlaps included).
 * Indices: an entry <= 0 (the class token, __remove_cls_token :192-196) or > num_patches is ignored -- never used as an index,
 * its pred row is skipped.  The entries of one image must be distinct (with a repeated entry either of its pred rows may win).
 * Limits, checked before any launch: image_size % patch_size == 0, batch * num_patches < 2^31, num_mask >= 1; fp32 images /
 * outputs 16-byte aligned and uint8 ones 4-byte (4 / 1 when patch_size or image_size is no multiple of 4), pred 4-byte.  scratch: mae_reconstruct_scratch_bytes(...) bytes, 256-byte aligned (-1 = arguments
 * outside the limits). */
int64_t mae_reconstruct_scratch_bytes(int32_t batch, int32_t in_chans, int32_t image_size, int32_t patch_size);
int mae_reconstruct_compose(const void* images, int32_t image_dtype, const float* pred, const int64_t* idx_mask,
                            int32_t batch, int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t num_mask,
                            float fill, int32_t out_dtype, void* recon, void* masked, float* stats,
                            void* scratch, int64_t scratch_bytes, void* stream);
/* MAEReconstructor.reconstruct_batch (:127-168) in one call on one stream: mae_engine_forward_encoder(images, idx_keep), then
 * mae_engine_forward_decoder(idx_keep, idx_mask), then mae_reconstruct_compose on its x_pred -- the same kernels, so x_pred is
 * what those two calls return.  workspace: mae_engine_workspace_bytes(batch, num_keep) bytes (the activations it saves are
 * simply unused, and those of any earlier forward are overwritten); x_pred (batch, num_mask, p*p*C) fp32 may be NULL (it then
 * lives in the workspace); recon / masked / stats / scratch / fill / out_dtype as mae_reconstruct_compose.  The engine must
 * predict pixels (pred_dim = 0).  Compose arguments are checked before anything is launched.
 * With norm_pix_loss the decoder's output lives in normalised space: x_pred still receives exactly what mae_engine_forward_decoder
 * returns, while recon / masked / stats are composed from its de-normalised copy (mae_norm_pix_restore), which is left in the
 * workspace's prediction slot (x_pred == NULL: de-normalised in place there).  stats is pixel-space error either way. */
int mae_engine_reconstruct(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                           const int64_t* idx_keep, const int64_t* idx_mask, int32_t batch, int32_t num_keep, int32_t num_mask,
                           float fill, int32_t out_dtype, void* workspace, int64_t workspace_bytes,
                           float* x_pred /* may be NULL */, void* recon, void* masked, float* stats,
                           void* scratch, int64_t scratch_bytes, void* stream);

/* Weighted k-NN probe on features (no reference counterpart; DINO's k-NN evaluation).
 * mae_knn_topk: for every query row the k bank rows of highest fp32 dot product, sorted by similarity descending, then bank
 *   index ascending; a NaN similarity is reported and sorted as -inf.  queries (num_queries, dim), bank (bank_size, dim) fp32,
 *   16-byte aligned, may be the same buffer; dim a multiple of 4 in [4, 4096]; 1 <= k <= min(256, bank_size);
 *   bank_size < 2^31.  The similarity of a pair is an fp32 fma chain in a fixed column order: it depends on the two rows
 *   only (not on num_queries, bank_size or how the bank is split).  topk_sim / topk_idx (num_queries, k).
 *   scratch: mae_knn_scratch_bytes(...) bytes, 256-byte aligned (-1 = arguments outside the limits).
 * mae_knn_vote: scores[q][c] = sum over j < k of [bank_labels[topk_idx[q][j]] == c] * exp(topk_sim[q][j] / temperature),
 *   summed in j order over the first k of k_stride columns; pred[q] = argmax (lowest class among equal scores).
 *   num_classes in [2, 128]; temperature > 0; scores (num_queries, num_classes) may be NULL.  A label outside
 *   [0, num_classes) is never used as an index: that query's scores are NaN and its pred is -1. */
int64_t mae_knn_scratch_bytes(int64_t num_queries, int64_t bank_size, int32_t dim, int32_t k);
int mae_knn_topk(const float* queries, int64_t num_queries, const float* bank, int64_t bank_size, int32_t dim, int32_t k,
                 float* topk_sim, int64_t* topk_idx, void* scratch, int64_t scratch_bytes, void* stream);
int mae_knn_vote(const float* topk_sim, const int64_t* topk_idx, int64_t num_queries, int32_t k_stride, int32_t k,
                 const int64_t* bank_labels, int32_t num_classes, float temperature, float* scores, int64_t* pred, void* stream);

/* mae_engine_optimizer_step with the EMA update of the target encoder fused into the AdamW sweep:
 * target[0 .. encoder_grad_elems) = m * target + (1 - m) * params_new (+ the bf16 operand copy in target_wcache).
 * max_norm = +inf disables clipping (I-JEPA trains unclipped). */
int mae_engine_optimizer_step_ema(mae_engine_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq,
                                  void* wcache, float lr, float beta1, float beta2, float eps, float weight_decay,
                                  float max_norm, int64_t step, float* stats_out, float* scratch, float* target_params,
                                  void* target_wcache, float ema_momentum, void* stream);

/* Per-kernel-class device timing with HIP events on `stream` (bench.py roofline): enable, run
 * steps, then read.  kind: index into mae_engine_timer_name().  Reading synchronises the events. */
int         mae_engine_timers_enable(mae_engine_t* e, int32_t on);
int32_t     mae_engine_timer_count(const mae_engine_t* e);
const char* mae_engine_timer_name(const mae_engine_t* e, int32_t kind);
int         mae_engine_timer_read(mae_engine_t* e, int32_t kind, double* total_ms, int64_t* launches,
                                  double* flops, double* bytes);
int         mae_engine_timers_reset(mae_engine_t* e);

/* ------------------------------------------------------------------------------------------
 * Single kernels (the pieces the engine is made of; exported for parity tests and reuse).
 * dtype arguments are MAE_F32 / MAE_BF16 and describe the `void*` activation tensors.
 * ---------------------------------------------------------------------------------------- */

/* LayerNorm(eps) forward over rows of x (fp32, rows x dim): y[r] = LN(x[row_map ? row_map[r] : r]).
 * mean/rstd: (rows) fp32 saved for backward. */
int mae_layernorm_fwd(const float* x, const int32_t* row_map, const float* gamma, const float* beta, float eps,
                      int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean, float* rstd, void* stream);
/* Same with the residual add fused in: v = x[row] + branch[row] (branch in y_dtype); x_out[row] = v (fp32); y = LN(v).
 * This is `x = x + attn(...)` / `x = x + mlp(...)` of timm Block followed by the next norm. */
int mae_add_layernorm_fwd(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                          const float* beta, float eps, int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean,
                          float* rstd, void* stream);
/* Backward: dx_io[row] = (accumulate ? dx_io[row] : 0) + dLN/dx ; dx_copy (dtype, may be NULL) gets the
 * same value in the activation dtype; dgamma/dbeta (dim) written.  partial: >= 2*1024*dim floats. */
int mae_layernorm_bwd(const void* dy, int32_t dy_dtype, const float* x, const int32_t* row_map, const float* gamma,
                      const float* mean, const float* rstd, int64_t rows, int32_t dim, int32_t accumulate,
                      float* dx_io, void* dx_copy, float* dgamma, float* dbeta, float* partial, void* stream);
/* The two calls above with a per-image scale (drop path).  The full-matrix row src (row_map[r], or r without a map) belongs to image
 * src / rows_per_image; that quotient indexes the scale vector, which the caller sizes (at least max(src) / rows_per_image + 1 floats).
 * rows_per_image <= 0 is refused before the launch; a NULL scale vector runs the unscaled call (same launches, same bits).
 *   forward : v = x[src] + image_scale[src / rows_per_image] * branch[src] in fp32; x_out[src] = v; y = LN(v).  A scale of exactly 0
 *             does not load the branch row: x_out[src] = x[src] bit for bit, whatever the branch holds.
 *   backward: dx_io, dgamma and dbeta as mae_layernorm_bwd; dx_copy[src] = copy_scale[src / rows_per_image] * dx_io[src], one fp32
 *             product of the value stored to dx_io, then the rounding to dx_copy's dtype.  copy_scale needs dx_copy. */
int mae_add_layernorm_fwd_scaled(const float* x, const void* branch, float* x_out, const int32_t* row_map, const float* gamma,
                                 const float* beta, float eps, int64_t rows, int32_t dim, int32_t y_dtype, void* y, float* mean,
                                 float* rstd, const float* image_scale, int32_t rows_per_image, void* stream);
int mae_layernorm_bwd_scaled(const void* dy, int32_t dy_dtype, const float* x, const int32_t* row_map, const float* gamma,
                             const float* mean, const float* rstd, int64_t rows, int32_t dim, int32_t accumulate,
                             float* dx_io, void* dx_copy, float* dgamma, float* dbeta, float* partial, const float* copy_scale,
                             int32_t rows_per_image, void* stream);

/* The classifier head alone (what mae_engine_classifier_* run after the encoder): feats (batch, seq_len, dim) in dtype,
 * head / labels / logits / loss_out / correct_out / head_grads as there.  d_feats (dtype, may be NULL): MAE_POOL_CLS ->
 * (batch, dim), the gradient of feats[:, 0] (every other row's gradient is zero); MAE_POOL_MEAN -> (batch, seq_len, dim).
 * scratch: mae_classifier_head_scratch_bytes(batch, num_classes, dim) bytes, 256-byte aligned. */
int64_t mae_classifier_head_scratch_bytes(int32_t batch, int32_t num_classes, int32_t dim);
int mae_classifier_head(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t pool,
                        const float* head, int32_t num_classes, const int64_t* labels, float grad_scale, float* logits,
                        float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats, void* scratch,
                        int64_t scratch_bytes, void* stream);
/* mae_classifier_head on feats whose seq_len rows do (with_cls = 1) or do not (0) start with a class-token row; pool as in
 * mae_engine_classifier_forward_ex (MAE_POOL_MEAN_PATCHES with with_cls = 1 needs seq_len >= 2).  d_feats is (batch, seq_len,
 * dim) for the mean pools, the class-token row exact zeros under MAE_POOL_MEAN_PATCHES.  Same scratch. */
int mae_classifier_head_ex(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t pool,
                           const float* head, int32_t num_classes, const int64_t* labels, float grad_scale, float* logits,
                           float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats, void* scratch,
                           int64_t scratch_bytes, void* stream);

/* mae_classifier_head_ex with the soft targets of mae_engine_classifier_loss_and_grads_soft (labels_b / lam / label_smoothing as
 * there).  With labels_b == NULL, lam == NULL and label_smoothing == 0 it is mae_classifier_head_ex: same launches, same bits. */
int mae_classifier_head_soft(const void* feats, int32_t dtype, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t pool,
                             const float* head, int32_t num_classes, const int64_t* labels, float grad_scale, float* logits,
                             float* loss_out, int32_t* correct_out, float* head_grads, void* d_feats, void* scratch,
                             int64_t scratch_bytes, const int64_t* labels_b, const float* lam, float label_smoothing, void* stream);

/* The linear probe of the MAE paper (A.1, Table 10; I-JEPA's probe is the same): BatchNorm1d(dim, affine=False, eps) over pooled
 * feature rows, mae_classifier_head on the normalised rows (MAE_F32, seq_len = 1, MAE_POOL_CLS), then LARS on the head.  Additive in
 * ABI v4; no reference counterpart.
 *
 * mae_batchnorm_fwd: x, y (rows, dim) fp32; y may be x itself (exactly in place), a partial overlap is refused.
 *   training != 0 (torch BatchNorm1d in train mode):
 *     mean[d] = sum_r x[r][d] / rows;  var[d] = sum_r (x[r][d] - mean[d])^2 / rows (biased);  rstd = 1 / sqrt(var + eps);
 *     y = (x - mean) * rstd;  running_mean = (1 - momentum) * running_mean + momentum * mean;
 *     running_var = (1 - momentum) * running_var + momentum * var * rows / (rows - 1) (the unbiased variance).
 *     rows >= 2.  running_mean and running_var (dim) may both be NULL: statistics are then not tracked.
 *   training == 0: y = (x - running_mean) / sqrt(running_var + eps); the running buffers are required and only read; rows >= 1;
 *     scratch is not used and may be NULL.
 *   mean_out / rstd_out (dim, may be NULL): the statistics y was formed with.
 *   The variance is centred, in fp32, in two column reductions: sum_r (x - x[0]) gives the mean, sum_r (x - mean)^2 the variance, each
 *   as row slices into partials that are added in a fixed order (no atomics): the order depends on (rows, dim) alone, so a call is
 *   bit-identical from run to run.  A constant column gives var == 0 and y == 0 exactly.  x is read three times, y written once.
 *   Limits, checked before any launch (a refused call launches nothing and writes nothing): dim % 4 == 0, 4 <= dim <= 1024;
 *   rows * dim < 2^40; 0 <= momentum <= 1; eps >= 0; every buffer 16-byte aligned; scratch_bytes >= mae_batchnorm_scratch_bytes(rows, dim)
 *   (-1 = rows / dim outside the limits).
 * mae_lars_step: the LARS of the MAE code base on a plain fp32 buffer of count elements (a multiple of 4, as for
 *   mae_engine_adamw_buffer; 0 is a no-op), 16-byte aligned:
 *     adapt = 1 (a weight matrix): dp = grads + weight_decay * params; pn = ||params||_2, un = ||dp||_2;
 *                                  q = (pn > 0 && un > 0) ? trust_coefficient * pn / un : 1;  dp *= q;
 *     adapt = 0 (a 1-D tensor: neither weight decay nor the trust ratio): dp = grads;
 *     then mu = momentum * mu + dp, params -= lr * mu.  No clip coefficient enters: the recipe trains unclipped.
 *   The norms are two-stage sums in a fixed order (no atomics) and q is formed on the device: nothing synchronises with the host.
 *   norms_out (2 floats, may be NULL) = pn, un before scaling (with adapt = 0: ||params||, ||grads||).  scratch: >= 4096 floats. */
int64_t mae_batchnorm_scratch_bytes(int64_t rows, int32_t dim);
int mae_batchnorm_fwd(const float* x, int64_t rows, int32_t dim, float eps, int32_t training, float momentum,
                      float* running_mean, float* running_var, float* y, float* mean_out /* may be NULL */,
                      float* rstd_out /* may be NULL */, void* scratch, int64_t scratch_bytes, void* stream);
int mae_lars_step(float* params, const float* grads, float* mu, int64_t count, int32_t adapt, float lr, float momentum,
                  float weight_decay, float trust_coefficient, float* norms_out /* may be NULL */, float* scratch, void* stream);

/* The statistics half of mae_batchnorm_fwd (additive in ABI v4): the same two centred column reductions and the same running-buffer
 * update by the same device code, so mean_out, rstd_out, running_mean and running_var get the bits mae_batchnorm_fwd gives them on
 * the same input; no normalising sweep and no y (x is read twice).  training == 0: mean_out = running_mean,
 * rstd_out = 1 / sqrt(running_var + eps).  mean_out and rstd_out are required; every other rule is mae_batchnorm_fwd's. */
int mae_batchnorm_stats(const float* x, int64_t rows, int32_t dim, float eps, int32_t training, float momentum, float* running_mean,
                        float* running_var, float* mean_out, float* rstd_out, void* scratch, int64_t scratch_bytes, void* stream);

/* The linear-probe sweep (additive in ABI v4; no reference counterpart): the G heads of a learning-rate /
 * weight-decay grid on the same BatchNorm output in one pass.  BatchNorm1d(affine=False) has no per-head state, so one
 * mae_batchnorm_fwd serves every head, and the heads are two GEMMs on the exact-fp32 MFMA over the stacked class index (g, c).
 *
 * mae_probe_sweep_head: y (rows, dim) fp32; heads = num_heads stacked buffers of HF = round_up(C * dim + C, 4) floats, each
 *   [W (C, dim) | b (C) | zero padding], the layout mae_classifier_head reads.  Per head g the call is mae_classifier_head on fp32 rows
 *   with seq_len = 1, MAE_POOL_CLS and grad_scale = 1:
 *     logits[g][b][c] = sum_d y[b][d] W_g[c][d] + b_g[c];  loss_out[g] = mean_b (logsumexp_c logits - logits[label]);
 *     correct_out[g] = #{b : argmax_c logits == label} (the first index among equal maxima);
 *     head_grads[g] = [dW = dlogits^T y | db = sum_b dlogits | zeros], dlogits = (softmax - onehot(label)) / rows.
 *   A label outside [0, C) is treated as mae_classifier_head's kernel treats it: it is never used as an index, the row's loss and
 *   its row of dlogits are NaN (so loss_out[g] and head g's gradients are NaN for every head) and the row does not count as correct.
 *   labels == NULL: logits only (logits is then required; loss_out / correct_out / head_grads are not written).
 *   head_grads == NULL: the evaluation call, nothing is written there.  logits == NULL: the logits stay in the scratch.
 *   The bits of head g's logits, loss, correct count and gradients do not depend on num_heads or on g's position in the stack: every
 *   output element is one fmaf chain whose order is fixed by (rows, dim) alone -- the forward walks dim in the order 0, 4, 1, 5, 2, 6,
 *   3, 7, 8, 12, ...; the weight gradient walks the rows of min(ceil(rows / 128), 16) batch slices [rows s / S, rows (s + 1) / S) in
 *   ascending order and the slices are added in order.  No atomics; a call is bit-identical from run to run.
 *   Limits, checked before any launch (a refused call launches nothing and writes nothing): dim % 4 == 0, 4 <= dim <= 1024;
 *   2 <= num_classes <= 128; 1 <= num_heads <= 64; rows >= 1, rows * num_heads * num_classes < 2^31; every buffer 16-byte aligned;
 *   labels come with loss_out and correct_out, head_grads with labels; scratch_bytes >= mae_probe_sweep_scratch_bytes (-1 = outside
 *   the limits).
 * mae_lars_step_groups: mae_lars_step on the num_groups <= 64 segments params + g * group_stride (count elements each; count and
 *   group_stride multiples of 4, group_stride >= count; grads and mu laid out alike) with per-group lr[g] and weight_decay[g].  Both
 *   are HOST arrays of num_groups floats that are copied into the kernel arguments: nothing is staged on the device and nothing
 *   synchronises.  Each group gets, bit for bit, what mae_lars_step gives on that segment alone (params, mu and norms: the same device
 *   code with the segment on blockIdx.y); the elements between the groups are not touched.  norms_out (num_groups, 2) may be NULL.
 *   scratch_floats >= 4096 * num_groups. */
int64_t mae_probe_sweep_scratch_bytes(int64_t rows, int32_t dim, int32_t num_classes, int32_t num_heads);
int mae_probe_sweep_head(const float* y, int64_t rows, int32_t dim, const float* heads, int32_t num_heads, int32_t num_classes,
                         const int64_t* labels /* may be NULL */, float* logits /* (G, rows, C), may be NULL */, float* loss_out /* G */,
                         int32_t* correct_out /* G */, float* head_grads /* (G, HF), may be NULL */, void* scratch, int64_t scratch_bytes,
                         void* stream);
int mae_lars_step_groups(float* params, const float* grads, float* mu, int32_t num_groups, int64_t group_stride, int64_t count,
                         int32_t adapt, const float* lr /* HOST, G */, const float* weight_decay /* HOST, G */, float momentum,
                         float trust_coefficient, float* norms_out /* (G, 2), may be NULL */, float* scratch, int64_t scratch_floats,
                         void* stream);

/* The attentive probe on cached tokens (additive in ABI v4; no reference counterpart).  x (batch, tokens, dim) fp32 is
 * the frozen encoder's output, heads | dim, hd = dim / heads; q (dim), Wk, Wv (dim, dim), no bias.  Behind BatchNorm1d(affine=False)
 * with statistics mean / rstd (dim) the definition is
 *     xh = (x - mean) rstd;  k, v = xh Wk^T, xh Wv^T;  s[b,t,h] = hd^-1/2 q[h] . k[b,t,h];  a = softmax over t;  p[b,h] = sum_t a v[b,t,h]
 * and the folded form below computes it without writing anything of the size of x, reading x once per pass:
 *   mae_attn_probe_fold       : uq[h][d] = rstd[d] * (hd^-1/2 * sum_j q[h hd + j] Wk[h hd + j][d])                        (heads, dim)
 *   mae_attn_pool_fwd         : s = (x - mean) . uq[h]; lse[b][h] = log sum_t exp s; a = exp(s - lse);
 *                               ybar[b][h][:] = sum_t a (x[b][t][:] - mean).  mean may be NULL (= 0).  One pass over x with a running
 *                               maximum and sum over token chunks; an image's ybar and lse do not depend on the batch it is part of
 *   mae_attn_probe_project    : p[b][h hd + j] = sum_d (Wv[h hd + j][d] rstd[d]) ybar[b][h][d]                             (batch, dim)
 *   mae_attn_probe_project_bwd: g[b][h][d] = rstd[d] * sum_j dp[b][h hd + j] Wv[h hd + j][d]                        (batch, heads, dim)
 *                               dwv[h hd + j][d] = rstd[d] * sum_b dp[b][h hd + j] ybar[b][h][d]
 *   mae_attn_pool_bwd         : delta = ybar[b][h] . g[b][h]; da = (x - mean) . g[b][h]; ds = exp(s - lse) (da - delta);
 *                               duq[h][:] = sum_{b,t} ds (x[b][t][:] - mean)                                              (heads, dim)
 *   mae_attn_probe_fold_bwd   : du = rstd duq[h]; dwk[h hd + j][:] = hd^-1/2 q[h hd + j] du; dq[h hd + j] = hd^-1/2 Wk[h hd + j] . du
 * No gradient flows to x or to the statistics.  The head on p is mae_classifier_head (MAE_F32, seq_len 1, MAE_POOL_CLS), whose d_feats
 * is dp.  Every sum has a fixed order that depends on the shape alone (image and batch slices into scratch, added in order; no
 * atomics), so a call is bit-identical from run to run.
 * Limits, checked before any launch (a refused call launches nothing and writes nothing): dim % 4 == 0, 4 <= dim <= 1024,
 * 1 <= heads <= 16, dim % heads == 0, batch >= 1, tokens >= 1, batch * tokens < 2^31; every buffer 16-byte aligned;
 * scratch_bytes >= the call's ..._scratch_bytes query (-1 = outside the limits). */
int mae_attn_pool_fwd(const float* x, const float* mean /* may be NULL */, const float* uq, int64_t batch, int64_t tokens, int32_t dim,
                      int32_t heads, float* ybar, float* lse, void* stream);
int64_t mae_attn_pool_bwd_scratch_bytes(int64_t batch, int64_t tokens, int32_t dim, int32_t heads);
int mae_attn_pool_bwd(const float* x, const float* mean /* may be NULL */, const float* uq, const float* lse, const float* ybar,
                      const float* g, int64_t batch, int64_t tokens, int32_t dim, int32_t heads, float* duq, void* scratch,
                      int64_t scratch_bytes, void* stream);
int mae_attn_probe_fold(const float* q, const float* wk, const float* rstd, int32_t dim, int32_t heads, float* uq, void* stream);
int mae_attn_probe_fold_bwd(const float* duq, const float* q, const float* wk, const float* rstd, int32_t dim, int32_t heads, float* dq,
                            float* dwk, void* stream);
int mae_attn_probe_project(const float* ybar, const float* rstd, const float* wv, int64_t batch, int32_t dim, int32_t heads, float* p,
                           void* stream);
int64_t mae_attn_probe_project_bwd_scratch_bytes(int64_t batch, int32_t dim, int32_t heads);
int mae_attn_probe_project_bwd(const float* dp, const float* ybar, const float* rstd, const float* wv, int64_t batch, int32_t dim,
                               int32_t heads, float* g, float* dwv, void* scratch, int64_t scratch_bytes, void* stream);

/* Epilogues of the GEMM family. */
enum {
  MAE_EPI_NONE  = 0,  /* out = acc (+bias)                                        */
  MAE_EPI_GELU  = 1,  /* out = acc+bias (pre-activation), out2 = gelu_erf(out)    */
  MAE_EPI_RESID = 2,  /* out(fp32) = resid(fp32) + acc + bias                     */
  MAE_EPI_DGELU = 3,  /* out = acc * gelu_erf'(aux[m][n])  (aux = saved pre-act)  */
  MAE_EPI_GELU_GRAD = 4, /* v = acc+bias rounded to the output type; out = gelu_erf'(v), out2 = gelu_erf(v): the forward
                            saves the derivative instead of the pre-activation, so backward only multiplies  */
  MAE_EPI_MUL   = 5,  /* out = acc * aux[m][n]                                  */
  MAE_EPI_GELU_ACT = 6 /* out = gelu_erf(acc+bias rounded to the output type): one output, for forward-only passes
                          (the I-JEPA target encoder never runs backward, so nothing but the activation is needed) */
};
/* out[M,N] = A[M,K] * W[N,K]^T (+ bias[N]) -- torch.nn.functional.linear.  A, W in `dtype`;
 * out/out2/aux in out_dtype (MAE_EPI_RESID: out and resid fp32). */
int mae_linear_fwd(const void* A, const void* W, const float* bias, int64_t M, int32_t N, int32_t K, int32_t dtype,
                   int32_t epilogue, int32_t out_dtype, void* out, void* out2, const void* aux_or_resid,
                   void* stream);
/* dW[N,K] = dY[M,N]^T * A[M,K] (fp32 out, written), db[N] = column sums of dY (may be NULL).
 * scratch: mae_linear_wgrad_scratch_bytes(M, N, K) bytes. */
int64_t mae_linear_wgrad_scratch_bytes(int64_t M, int32_t N, int32_t K);
int mae_linear_wgrad(const void* dY, const void* A, int64_t M, int32_t N, int32_t K, int32_t dtype, float* dW,
                     float* db, void* scratch, void* stream);

/* Two weight gradients over the same M rows in one launch (the engine pairs a block's fc2 + fc1 and proj + qkv:
 * torch.autograd's dW = dY^T X of two nn.Linear, timm Block / Attention).  Same results contract as two
 * mae_linear_wgrad calls (fp32 dW / db written); falls back to exactly those when a shape is outside the
 * ring kernel.  scratch >= mae_linear_wgrad_pair_scratch_bytes. */
int64_t mae_linear_wgrad_pair_scratch_bytes(int64_t M, int32_t N0, int32_t K0, int32_t N1, int32_t K1);
int mae_linear_wgrad_pair(const void* dY0, const void* A0, int32_t N0, int32_t K0, float* dW0, float* db0,
                          const void* dY1, const void* A1, int32_t N1, int32_t K1, float* dW1, float* db1,
                          int64_t M, int32_t dtype, void* scratch, void* stream);

/* Multi-head self-attention core of timm Attention (F.scaled_dot_product_attention, no mask, no dropout).
 * qkv: (batch, T, 3, H, hd) in `dtype` as the qkv Linear emits it; out: (batch, T, H*hd) in `dtype`;
 * lse: (batch, H, T) fp32 log-sum-exp of the scaled scores, saved for backward. */
int mae_attention_fwd(const void* qkv, int32_t batch, int32_t T, int32_t H, int32_t hd, int32_t dtype, void* out,
                      float* lse, void* stream);
int mae_attention_bwd(const void* qkv, const void* out, const void* d_out, const float* lse, int32_t batch,
                      int32_t T, int32_t H, int32_t hd, int32_t dtype, void* d_qkv, void* stream);

/* Weighted column sum of the attention probabilities of one block, from its qkv (layout as above; V is not read):
 *     P_b,h[t][j] = softmax_j(hd^-1/2 q_t . k_j)
 *     per_head[b * per_head_stride + h * T + j] = sum_t row_weight[b][t] P_b,h[t][j]              (fp32; stride in floats)
 *     mixed[b][j] = row_weight[b][j] / 2 + (1 / (2 H)) sum_h per_head[b][h][j]                    ((batch, T) fp32: one rollout step)
 *   Either output may be NULL, not both; each holds the same bits whether or not the other is asked for.  mixed must not overlap
 *   row_weight.  All arithmetic is fp32: scores by fused multiply-adds over d in index order, the row maximum subtracted before the
 *   exponential, every row divided by its own sum (no saved log-sum-exp).  A row whose weight is exactly 0 is skipped and its q is
 *   not read.  No atomics: every sum has an order fixed by the shape, and an image's result does not depend on its batch.
 *   Limits (checked before the launch; a refused call writes nothing): hd in {16, 24, 32, 48, 64}; 1 <= H <= 16; batch * T < 2^31;
 *   T <= mae_attention_colsum_max_tokens(hd, dtype) (what the LDS layout of the keys allows: 512 for every supported pair; -1 for an
 *   unsupported one); qkv, row_weight and mixed 16-byte aligned; per_head a float pointer with per_head_stride >= H * T, so that a
 *   slice of a (batch, n, H, T) buffer can be written in place whatever H * T is. */
int32_t mae_attention_colsum_max_tokens(int32_t hd, int32_t dtype);
int mae_attention_colsum(const void* qkv, int32_t dtype, int32_t batch, int32_t T, int32_t H, int32_t hd, const float* row_weight,
                         float* per_head, int64_t per_head_stride, float* mixed, void* stream);

/* Exact t-SNE of n feature rows in the plane (additive in ABI v4; no reference counterpart).  Everything is fp32; every
 * sum has an order fixed by (n, dim) alone and there are no atomics, so a call is bit-identical from run to run; nothing synchronises
 * with the host and every buffer is the caller's.  Limits, refused by name before any pointer is touched: 8 <= n <= 16384,
 * 1 <= dim <= 8192, 1 <= perplexity < n - 1.
 *   mae_tsne_pitch(n)        round_up(n, 4), the row pitch of P in floats (-1 outside the limits).  P is (n, pitch), 16-byte aligned,
 *                            with zeros in the columns [n, pitch).
 *   mae_tsne_scratch_bytes   the scratch of mae_tsne_gradient / mae_tsne_step (-1 outside the limits).
 *   mae_tsne_affinities      d_ij = sum_k (x_ik - x_jk)^2 (the difference form, one fused multiply-add per k in the order of k);
 *                            per row sklearn's _binary_search_perplexity on d_ij less the row's minimum over j != i: beta from 1,
 *                            doubled or halved until bracketed, then bisected, at most 100 steps, until |H_i - log(perplexity)| <= 1e-5,
 *                            H_i = log sum_j e^(-beta d_ij) + beta sum_j d_ij p_j|i over j != i; p_j|i = e^(-beta_i d_ij) / sum;
 *                            P_ij = (p_j|i + p_i|j) / (2 n), symmetric bit for bit, diagonal 0.  The symmetrisation is a launch of
 *                            its own, in place.  sqdist (n, n), beta (n) and p_cond (n, n), all unpadded, may each be NULL.
 *   mae_tsne_gradient        with w_ij = 1 / (1 + |y_i - y_j|^2) (v_rcp_f32): a_i = sum_j p_ij w_ij (y_i - y_j), r_i = sum_j w_ij^2
 *                            (y_i - y_j), Z = sum_i sum_{j != i} w_ij, grad_i = 4 (alpha a_i - r_i / Z), one pass over P.  kl (one
 *                            float, may be NULL) = sum_{i != j} p_ij (log p_ij - log w_ij) + log Z with 0 log 0 = 0; P is taken as it
 *                            is given (alpha is not applied to it).  grad (n, 2) is required.
 *   mae_tsne_update          sklearn's _gradient_descent step per coordinate, every operation rounded once (no contraction):
 *                            gains = max(update * grad < 0 ? gains + 0.2f : gains * 0.8f, min_gain);
 *                            update = momentum * update - learning_rate * (grad * gains);  y = y + update.
 *   mae_tsne_step            mae_tsne_gradient followed by mae_tsne_update, bit for bit, in two launches instead of three.
 *   y, update, gains, grad (n, 2) and scratch must be 16-byte aligned. */
int32_t mae_tsne_pitch(int32_t n);
int64_t mae_tsne_scratch_bytes(int32_t n, int32_t dim);
int mae_tsne_affinities(const float* x, int32_t n, int32_t dim, float perplexity, float* P, float* sqdist /* may be NULL */,
                        float* beta /* may be NULL */, float* p_cond /* may be NULL */, void* stream);
int mae_tsne_gradient(const float* P, const float* y, int32_t n, float alpha, float* grad, float* kl /* may be NULL */, void* scratch,
                      int64_t scratch_bytes, void* stream);
int mae_tsne_update(float* y, float* update, float* gains, const float* grad, int32_t n, float momentum, float learning_rate,
                    float min_gain, void* stream);
int mae_tsne_step(const float* P, float* y, float* update, float* gains, int32_t n, float alpha, float momentum, float learning_rate,
                  float min_gain, float* grad, float* kl /* may be NULL */, void* scratch, int64_t scratch_bytes, void* stream);

/* UMAP of n feature rows in the plane (McInnes et al.; umap-learn 0.5's defaults; additive in ABI v4; no reference counterpart;
 * DESIGN.md 11.4).  Everything is fp32; every sum has an order fixed by the shapes alone and there are no atomics, so a call is
 * bit-identical from run to run; nothing synchronises with the host and every buffer is the caller's.  Limits, refused by name before
 * any pointer is touched: 8 <= n <= 16384, 1 <= dim <= 8192, 2 <= n_neighbors <= 64, n_neighbors < n, 1 <= rate <= 16, 0 <= t < 2^24.
 *   mae_umap_scratch_bytes   the scratch of mae_umap_fuzzy_knn: the (n, round_up(n, 4)) squared distances and two rows (-1 outside the
 *                            limits).  16-byte aligned.
 *   mae_umap_fuzzy_knn       d_ij = sqrt(sum_c (x_ic - x_jc)^2): the difference form of mae_tsne_affinities (one fused multiply-add per
 *                            column in column order), then one correctly rounded square root.  Row i of knn_idx / knn_dist (n, k) holds
 *                            the k smallest d_ij, the point itself included, by distance ascending, then index ascending.
 *                            rho_i = the first entry > 0 (0 if none).  sigma_i by umap-learn's smooth_knn_dist: lo = 0, hi = inf,
 *                            mid = 1; at most 64 steps; psum = sum_{r = 1 .. k - 1} e^(-(max(d_ir - rho_i, 0) / mid)); stop when
 *                            |psum - log2 k| < 1e-5; psum above: hi = mid, mid = (lo + hi) / 2; else lo = mid, and mid doubles while
 *                            hi = inf, else mid = (lo + hi) / 2.  Floor: sigma_i >= 1e-3 x the row's mean distance when rho_i > 0, else
 *                            >= 1e-3 x the mean of all n k distances (the rows' sums added in a fixed order).  memb (n, k) = 0 for the
 *                            point itself, 1 if d - rho <= 0 or sigma = 0, else e^(-((d - rho) / sigma)).  Exponentials by v_exp_f32.
 *   mae_umap_epoch           epoch t of the synchronous layout over a CSR graph of E directed edges: row_ptr (n + 1), col / eps / next
 *                            (E); row_ptr ascending from 0, the caller's word is taken for it; a column outside [0, n) is clamped.
 *                            Edge e of row i fires iff next[e] <= t.  A firing edge adds to row i, from y_in alone,
 *                              2 clip(c (y_i - y_j)),  j = col[e],  c = -2 a b d2^(b - 1) / (a d2^b + 1),  d2 = |y_i - y_j|^2, and for
 *                              s = 0 .. rate - 1:  clip(c (y_i - y_k)),  c = 2 gamma b / ((0.001 + d2) (a d2^b + 1)),  d2 = |y_i - y_k|^2,
 *                            clip per coordinate to [-4, 4]; a term with d2 = 0, or with k = i, is 0.  The negative sample is
 *                              k = (uint64(h) * n) >> 32,  h = mix(mix(seed, t), 16 e + s),  mix(s, i) = fmix32(fmix32(i + 0x9E3779B9) ^ s)
 *                            in uint32 arithmetic, fmix32 murmur3's finaliser (h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13;
 *                            h *= 0xC2B2AE35; h ^= h >> 16), e the edge's index in col.  16 e + s < 2^25 for E <= 2 n k <= 2^21: the key
 *                            never wraps.  y_out[i] = fma(alpha, sum_i, y_in[i]) for every row; next[e] += eps[e] (one fp32 add) on the
 *                            edges that fired.  The sum's order depends on the row's degree and the rate alone.  y_in is not written
 *                            and must not be y_out; y_in and y_out (n, 2) 16-byte aligned. */
int64_t mae_umap_scratch_bytes(int32_t n, int32_t dim, int32_t n_neighbors);
int mae_umap_fuzzy_knn(const float* x, int32_t n, int32_t dim, int32_t n_neighbors, int32_t* knn_idx, float* knn_dist, float* memb,
                       float* rho, float* sigma, void* scratch, int64_t scratch_bytes, void* stream);
int mae_umap_epoch(const float* y_in, float* y_out, const int32_t* row_ptr, const int32_t* col, const float* eps, float* next,
                   int32_t n, float a, float b, float gamma, float alpha, int32_t t, int32_t rate, uint32_t seed, void* stream);

/* Token and pixel movement between those pieces, and the losses that read the image.  Index arguments are int32, as the kernels
 * take them; token id 0 is the class token, id t >= 1 is patch t - 1 (row-major over the patch grid).  Unless a function says
 * otherwise the ids must lie in [0, seq_len): nothing here range-checks them on the device.  `partial` is scratch of
 * >= 512 * dim floats.  Column sums are two-stage, in a fixed order (no atomics): bit-identical from run to run. */

/* Rows of the patch-embedding GEMM: out (batch * num_keep, C*p*p) in out_dtype, row (b, j) = patch tok32[b][j] - 1 of image b in
 * conv-weight order (c, py, px); a class-token id (<= 0) gives a zero row.  images as mae_engine_forward_encoder (MAE_U8: normalised
 * in the read; needs patch_size % 4 == 0, at most 64 patches per side and C * p * image_size <= 96 KiB, else an error before
 * the launch).  MAE_F32 images: ids in [0, num_patches] (not clamped). */
int mae_gather_patches(const void* images, int32_t image_dtype, const int32_t* tok32, int32_t batch, int32_t num_keep,
                       int32_t in_chans, int32_t image_size, int32_t patch_size, int32_t out_dtype, void* out, void* stream);
/* In place on x (rows, dim) fp32: x[r] = (tok32[r] == 0 ? cls : x[r]) + pos[tok32[r]] -- one fp32 addition.  dim % 4 == 0. */
int mae_assemble_visible(float* x, const int32_t* tok32, const float* cls, const float* pos, int64_t rows, int32_t dim,
                         void* stream);
/* Its adjoint: dtok (rows, dim) in dtype = dx with the class-token rows (tok32[r] == 0) replaced by exact zeros; dcls (dim)
 * fp32 = the sum of those rows.  dx fp32; dim % 4 == 0, dim <= 1024. */
int mae_visible_grad_split(const float* dx, const int32_t* tok32, int64_t rows, int32_t dim, int32_t dtype, void* dtok,
                           float* dcls, float* partial, void* stream);
/* inv (batch, seq_len): inv[b][keep32[b][j]] = j, every other entry -1 (ids outside [0, seq_len) are ignored). */
int mae_build_inverse(const int32_t* keep32, int32_t batch, int32_t num_keep, int32_t seq_len, int32_t* inv, void* stream);
/* rows[b * n_per + j] = b * seq_len + clamp(idx32[b][j], 0, seq_len - 1): rows of the (batch * seq_len) decoder matrix. */
int mae_build_row_map(const int32_t* idx32, int32_t batch, int32_t n_per, int32_t seq_len, int32_t* rows, void* stream);
/* Decoder input: out[b][t] (fp32) = (inv[b][t] >= 0 ? xdec[b * num_keep + inv[b][t]] : mask_token) + pos[t]; xdec in dtype,
 * widened to fp32 before the one fp32 addition.  dim % 4 == 0, dim <= 1024, batch * seq_len < 2^31. */
int mae_decoder_assemble(const void* xdec, int32_t dtype, const int32_t* inv, const float* mask_token, const float* pos,
                         int32_t batch, int32_t num_keep, int32_t seq_len, int32_t dim, float* out, void* stream);
/* Its adjoint: d_xdec[b * num_keep + inv[b][t]] (dtype) = dx[b][t] for every t with inv >= 0 (rows no inv entry names are not
 * written); d_mask_token (dim) fp32 = the sum of the rows with inv < 0 (exact zeros when there are none). */
int mae_decoder_assemble_bwd(const float* dx, const int32_t* inv, int32_t batch, int32_t num_keep, int32_t seq_len, int32_t dim,
                             int32_t dtype, void* d_xdec, float* d_mask_token, float* partial, void* stream);
/* Exact zeros in every row of dres (fp32) and dres_c (dtype), both (rows, dim), that the prediction head never saw: rows with
 * inv[row] >= 0, or with inv == NULL the first seq_len - num_pred rows of every sequence of seq_len.  No other row is touched. */
int mae_zero_unpredicted_rows(const int32_t* inv_or_null, int64_t rows, int32_t seq_len, int32_t num_pred, int32_t dim,
                              int32_t dtype, float* dres, void* dres_c, void* stream);
/* mae_mse_loss between pred (batch, num_mask, p*p*C) fp32 and the patches mask32 of images in (py, px, c) order, never written
 * to memory: n = batch * num_mask * p*p*C, d_pred (may be NULL) in d_pred_dtype.  One rule for every variant (band walk over
 * float images, band walk over uint8 images, per-pixel gather): entry t reads patch clamp(t - 1, 0, num_patches - 1).
 *   path = 0: what the engine launches (MAE_U8: the uint8 band walk, or an error when patch_size % 4 != 0, more than 64 patches
 *             per side or a band beyond the LDS; MAE_F32: the band walk where it applies, else the per-pixel gather);
 *   path = 1: the per-pixel gather, MAE_F32 images only.
 * scratch: >= 4096 floats. */
int mae_mse_loss_from_images(const float* pred, const void* images, int32_t image_dtype, const int32_t* mask32, int32_t batch,
                             int32_t num_mask, int32_t in_chans, int32_t image_size, int32_t patch_size, float grad_scale,
                             float* loss, void* d_pred /* may be NULL */, int32_t d_pred_dtype, float* scratch, int32_t path,
                             void* stream);
/* I-JEPA predictor input: num_blocks sequences per image of num_context + block_tokens rows,
 * out[(b, blk, t)] (fp32) = t < num_context ? xdec[b * num_context + t] + pos[ctx32[b][t]]
 *                                           : mask_token + pos[tgt32[b][blk][t - num_context]]   (ids clamped into [0, seq_len)). */
int mae_predictor_assemble(const void* xdec, int32_t dtype, const int32_t* ctx32, const int32_t* tgt32, const float* mask_token,
                           const float* pos, int32_t batch, int32_t num_context, int32_t num_blocks, int32_t block_tokens,
                           int32_t seq_len, int32_t dim, float* out, void* stream);
/* Its adjoint: d_xdec[b * num_context + t] (dtype) = sum over blk (ascending) of dx[(b, blk, t)]; d_mask_token (dim) fp32 = the sum
 * of every mask-token row. */
int mae_predictor_assemble_bwd(const float* dx, int32_t batch, int32_t num_context, int32_t num_blocks, int32_t block_tokens,
                               int32_t dim, int32_t dtype, void* d_xdec, float* d_mask_token, float* partial, void* stream);
/* rows[seq * num_pred + j] = seq * seq_len + (seq_len - num_pred) + j: the last num_pred rows of every sequence. */
int mae_build_tail_row_map(int32_t seqs, int32_t seq_len, int32_t num_pred, int32_t* rows, void* stream);
/* rows[i] = (i / per_image) * num_patches + clamp(tok32[i] - 1, 0, num_patches - 1). */
int mae_rows_from_tokens(const int32_t* tok32, int32_t batch, int32_t per_image, int32_t num_patches, int32_t* rows, void* stream);
/* torch.nn.functional.smooth_l1_loss (beta = 1, mean) over n elements (n % 4 == 0) and its gradient:
 * d_pred (may be NULL, d_pred_dtype) = clamp(pred - target, -1, 1) * (grad_scale / n).  scratch: >= 4096 floats. */
int mae_smooth_l1_loss(const float* pred, const float* target, int64_t n, float grad_scale, float* loss,
                       void* d_pred /* may be NULL */, int32_t d_pred_dtype, float* scratch, void* stream);

/* The kernels only the engine launches, on caller buffers (parity tests and reuse).  Additive in ABI v4.  Each call launches exactly
 * what the engine launches for the same arguments.  Every check below is made before any launch: a refused call launches nothing
 * and writes nothing.  dtype arguments are MAE_F32 or MAE_BF16, anything else (MAE_U8 included) is refused.
 *
 * mae_full_grad_split: the embedding gradient of a full sequence in one pass over dx (batch, seq_len, dim) fp32.
 *   with_cls = 1 (row 0 of every image is the class token):
 *     dtok (batch, seq_len, dim) in dtype = dx (MAE_BF16: rounded to nearest even), row 0 of every image +0.0;
 *     dpos (seq_len, dim) fp32: dpos[t][d] = sum_b dx[b][t][d];  dcls (dim) fp32 = dpos[0], bit for bit.
 *   with_cls = 0 (patch-only sequence: seq_len patch rows, row t is token t + 1): dtok = dx, no row zeroed;
 *     dpos holds (seq_len + 1, dim) floats: dpos[t + 1][d] = sum_b dx[b][t][d], dpos[0] = +0.0;  dcls = +0.0.
 *   The sum runs over S = mae_full_grad_split_partial_floats / (seq_len * dim) batch slices [batch * s / S, batch * (s + 1) / S),
 *   each in ascending order, and the slices' partials are then added in a fixed order (no atomics): bit-identical from run to run.
 *   S = max(1, min(batch, 64, ceil(2048 / ceil(seq_len * (dim / 4) / 256)))).
 *   partial: scratch of >= mae_full_grad_split_partial_floats(batch, seq_len, dim) floats (-1 = arguments outside the limits).
 *   Limits: dim % 4 == 0, 4 <= dim <= 1024, batch * seq_len < 2^31, no NULL buffer.  Buffers 16-byte aligned.
 * mae_zero_token_rows: +0.0 in every row r of dres (fp32) and dres_c (dtype), both (rows, dim), with r % seq_len != 0; the rows
 *   r % seq_len == 0 (the class tokens) keep their bits.  rows need not be a multiple of seq_len.  dim as above.
 * mae_features_pool: out (batch, dim) fp32 from x_mid (fp32) and branch (branch_dtype), both (batch, seq_len, dim):
 *     v = fl32(x_mid + branch);  y[t] = LayerNorm(v[t]; gamma, beta, eps) in fp32 (biased variance, 1 / sqrt(var + eps));
 *     f = sum_{t in [row_lo, row_hi)} y[t] / (row_hi - row_lo);  normalize = MAE_FEAT_L2: out = f / (||f||_2 + 1e-8), else out = f.
 *   One block per image; wave w of four adds rows row_lo + w, row_lo + w + 4, ... and the four sums are added in wave order, so an
 *   image's result does not depend on batch.  Only the pooled rows are read.  Limits: dim as above, 0 <= row_lo < row_hi <= seq_len;
 *   out 4-byte aligned.
 * mae_features_tap: the same kernel by (with_cls, pool) with a row stride on the output: image b's feature goes to
 *     out + b * out_row_stride (floats).  Rows pooled: MAE_POOL_CLS row 0; MAE_POOL_MEAN every row; MAE_POOL_MEAN_PATCHES rows
 *     [with_cls, seq_len); each with mae_features_pool's arithmetic order, so the slice holds its bits.  MAE_POOL_CLS_MEAN_PATCHES:
 *     W = 2 dim, out[0, dim) = the MAE_POOL_CLS result, out[dim, 2 dim) = the MAE_POOL_MEAN_PATCHES result, bit for bit, from one
 *     pass over the rows; MAE_FEAT_L2 normalises each half on its own.  Nothing outside [0, W) of a slice is written.
 *   Limits (checked before the launch): dim as above; MAE_POOL_CLS and MAE_POOL_CLS_MEAN_PATCHES need with_cls = 1;
 *   MAE_POOL_CLS_MEAN_PATCHES, and MAE_POOL_MEAN_PATCHES with with_cls = 1, need seq_len >= 2; out_row_stride >= W and a multiple
 *   of 4; out 16-byte aligned.
 * mae_cast: dst[i] = src[i] converted, i < n: fp32 -> bf16 rounds to nearest even (a NaN stays a quiet NaN), bf16 -> fp32 is
 *   exact, equal types copy.  n > 0.
 * mae_add_rows_pos: out[r] = fl32(x[r] + pos[r % seq_len]) for r < rows; x, out (rows, dim), pos (seq_len, dim) fp32.
 *   dim % 4 == 0, dim >= 4.
 * mae_add_into: dst[i] (dst_dtype) = fl32(dst[i] + src[i]) (MAE_BF16: dst widened, the fp32 sum rounded to nearest even); src fp32.
 * mae_linear_dgrad: out[M,K] = dY[M,N] * W[N,K] -- the input gradient of torch.nn.functional.linear -- by the exact-fp32 tiled
 *   kernel for every dtype: one fmaf chain over n = 0 .. N - 1 in ascending order per output (bf16 operands widened), then
 *     MAE_EPI_NONE: out = acc;  MAE_EPI_DGELU: out = acc * gelu_erf'(aux[m][k]);  MAE_EPI_MUL: out = acc * aux[m][k];
 *   any other epilogue is refused.  dY, W in dtype; out and aux (M, K) in out_dtype; fp32 operands with a bf16 output are refused.
 *   The engine launches it with fp32 operands only (bf16 dgrads go through mae_linear_fwd's kernels on a transposed weight copy).
 *   M <= 64 * 65535. */
int64_t mae_full_grad_split_partial_floats(int32_t batch, int32_t seq_len, int32_t dim);
int mae_full_grad_split(const float* dx, int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t dtype, void* dtok,
                        float* dpos, float* dcls, float* partial, void* stream);
int mae_zero_token_rows(int64_t rows, int32_t seq_len, int32_t dim, int32_t dtype, float* dres, void* dres_c, void* stream);
int mae_features_pool(const float* x_mid, const void* branch, int32_t branch_dtype, const float* gamma, const float* beta, float eps,
                      int32_t batch, int32_t seq_len, int32_t dim, int32_t row_lo, int32_t row_hi, int32_t normalize, float* out,
                      void* stream);
int mae_features_tap(const float* x_mid, const void* branch, int32_t branch_dtype, const float* gamma, const float* beta, float eps,
                     int32_t batch, int32_t seq_len, int32_t dim, int32_t with_cls, int32_t pool, int32_t normalize, float* out,
                     int64_t out_row_stride, void* stream);
int mae_cast(const void* src, int32_t src_dtype, void* dst, int32_t dst_dtype, int64_t n, void* stream);
int mae_add_rows_pos(const float* x, const float* pos, int64_t rows, int32_t seq_len, int32_t dim, float* out, void* stream);
int mae_add_into(const float* src, void* dst, int32_t dst_dtype, int64_t n, void* stream);
int mae_linear_dgrad(const void* dY, const void* W, int64_t M, int32_t N, int32_t K, int32_t dtype, int32_t epilogue,
                     int32_t out_dtype, void* out, const void* aux, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAE_HIP_H */
