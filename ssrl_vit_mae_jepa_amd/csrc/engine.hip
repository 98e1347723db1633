// The MAE pretrain-step engine: parameter arena, workspace plan and the launch sequences of
// forward_encoder / forward_decoder / backward / optimizer step.
// Reference control flow: src/models/mae.py:54-94 (forward), src/training/mae.py:45-65 (step),
// scripts/training/pretrain_mae.py:124-125 (clip).  Everything here only enqueues kernels on the caller's stream.
#include <string>
#include <vector>
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <cstdint>
#include "kernels.h"

namespace mae {

// ---------------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------------
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int hip_fail(hipError_t err, const char* what, const char* file, int line) {
  set_error("HIP error %d (%s) at %s:%d: %s", (int)err, hipGetErrorString(err), file, line, what);
  return 2;
}

// ---------------------------------------------------------------------------------------------------
// parameters
// ---------------------------------------------------------------------------------------------------
struct ParamInfo {
  std::string name;
  int64_t offset = 0, numel = 0;
  int ndim = 0;
  int64_t shape[4] = {1, 1, 1, 1};
  int flags = 0;
  int64_t t_off = -1;  // element offset of the transposed bf16 copy inside the wcache transposed region
};

struct BlockRefs {  // indices into params
  int ln1_w, ln1_b, qkv_w, qkv_b, proj_w, proj_b, ln2_w, ln2_b, fc1_w, fc1_b, fc2_w, fc2_b;
};

enum TimerKind { TK_LINEAR = 0, TK_WGRAD, TK_ATTN_FWD, TK_ATTN_BWD, TK_LN_FWD, TK_LN_BWD, TK_DATA, TK_LOSS, TK_OPTIM, TK_COUNT };
static const char* kTimerNames[TK_COUNT] = {"linear_nt", "linear_wgrad", "attention_fwd", "attention_bwd", "layernorm_fwd",
                                            "layernorm_bwd", "token_data_movement", "mse_loss", "clip_adamw"};

struct TimerSlot {
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
  size_t used = 0;
  double flops = 0, bytes = 0;
};

}  // namespace mae

using namespace mae;

struct mae_engine {
  mae_config_t cfg;
  int act = MAE_F32;
  int D, depth, H, Dd, dd, Hd, P, L, G, C, img, p, mlp;
  int PO;  // width of the prediction head: P (MAE pixels) or cfg.pred_dim (I-JEPA: the encoder width)
  std::vector<ParamInfo> params;
  int64_t arena_elems = 0, trainable_elems = 0, trans_elems = 0;
  int i_enc_mask, i_cls, i_pos, i_patch_w, i_patch_b, i_norm_w, i_norm_b;
  int i_dec_mask, i_dec_pos, i_de_w, i_de_b, i_dn_w, i_dn_b, i_pred_w, i_pred_b;
  std::vector<BlockRefs> enc, dec;
  bool timers_on = false;
  TimerSlot timers[TK_COUNT];
  PartialsTable ln_tab;  // LayerNorm dgamma / dbeta second stages queued by the current backward pass
};

namespace mae {

static int add_param(mae_engine* e, const std::string& name, std::initializer_list<int64_t> shape, int flags) {
  ParamInfo pi;
  pi.name = name;
  pi.ndim = (int)shape.size();
  pi.numel = 1;
  int i = 0;
  for (int64_t s : shape) { pi.shape[i++] = s; pi.numel *= s; }
  pi.flags = flags;
  e->params.push_back(pi);
  return (int)e->params.size() - 1;
}

static BlockRefs add_block(mae_engine* e, const std::string& pfx, int d, int mlp) {
  const int T = MAE_PARAM_TRAINABLE, M = MAE_PARAM_TRAINABLE | MAE_PARAM_MATRIX;
  BlockRefs r;
  r.ln1_w = add_param(e, pfx + ".norm1.weight", {d}, T);
  r.ln1_b = add_param(e, pfx + ".norm1.bias", {d}, T);
  r.qkv_w = add_param(e, pfx + ".attn.qkv.weight", {3 * (int64_t)d, d}, M);
  r.qkv_b = add_param(e, pfx + ".attn.qkv.bias", {3 * (int64_t)d}, T);
  r.proj_w = add_param(e, pfx + ".attn.proj.weight", {d, d}, M);
  r.proj_b = add_param(e, pfx + ".attn.proj.bias", {d}, T);
  r.ln2_w = add_param(e, pfx + ".norm2.weight", {d}, T);
  r.ln2_b = add_param(e, pfx + ".norm2.bias", {d}, T);
  r.fc1_w = add_param(e, pfx + ".mlp.fc1.weight", {(int64_t)mlp * d, d}, M);
  r.fc1_b = add_param(e, pfx + ".mlp.fc1.bias", {(int64_t)mlp * d}, T);
  r.fc2_w = add_param(e, pfx + ".mlp.fc2.weight", {d, (int64_t)mlp * d}, M);
  r.fc2_b = add_param(e, pfx + ".mlp.fc2.bias", {d}, T);
  return r;
}

// ---------------------------------------------------------------------------------------------------
// workspace plan: byte offsets of every saved activation / scratch buffer for (B, k)
// ---------------------------------------------------------------------------------------------------
struct LayerBufs {
  int64_t x_mid, ln1, mean1, rstd1, qkv, lse, att, ln2, mean2, rstd2, fc1_pre, fc1_act;
};

struct Plan {
  int B, k, m;
  int dec_B, dec_T;  // decoder / predictor attention batch and sequence length: (B, L) for MAE, (B * nblk, k + m) for I-JEPA
  int64_t Me, Md, Mp;
  int64_t keep32, mask32, inv, pred_rows;
  int64_t patchA;
  std::vector<int64_t> enc_x, dec_x;
  std::vector<LayerBufs> enc, dec;
  int64_t enc_norm, enc_mean, enc_rstd, xdec, dec_norm, dec_mean, dec_rstd, pred;
  // backward scratch
  int64_t branch_a, branch_b;  // bf16/fp32 outputs of the attention / MLP branches (added by the next LayerNorm kernel)
  int64_t dpred, d_decn, dres, dres_c, d_ln, d_att, d_qkv, d_hidden, d_xdec, dtok;
  int64_t ln_partial, ln_partial_stride, split_partial, wgrad_scratch, loss_scratch;
  int64_t total;
};

// dec_B sequences of dec_T tokens go through the decoder stack, m_seq of them per sequence reach the prediction head
static Plan make_plan_ex(const mae_engine* e, int B, int k, int dec_B, int dec_T, int m_seq) {
  Plan pl;
  pl.B = B; pl.k = k; pl.m = m_seq;
  pl.dec_B = dec_B; pl.dec_T = dec_T;
  pl.Me = (int64_t)B * k; pl.Md = (int64_t)dec_B * dec_T; pl.Mp = (int64_t)dec_B * m_seq;
  const int64_t as = (int64_t)dtype_size(e->act);
  int64_t off = 0;
  auto take = [&](int64_t bytes) { const int64_t o = off; off += round_up(std::max<int64_t>(bytes, 4), 256); return o; };
  pl.keep32 = take(pl.Me * 4);
  pl.mask32 = take(pl.Mp * 4);
  pl.inv = take(pl.Md * 4);
  pl.pred_rows = take(pl.Mp * 4);
  pl.patchA = take(pl.Me * e->P * as);
  auto layers = [&](int n, int64_t M, int d, int heads, int T, std::vector<int64_t>& xs, std::vector<LayerBufs>& ls) {
    const int64_t seqs = M / std::max(T, 1);
    xs.resize(n + 1);
    ls.resize(n);
    xs[0] = take(M * d * 4);
    for (int i = 0; i < n; ++i) {
      LayerBufs& b = ls[i];
      b.ln1 = take(M * d * as); b.mean1 = take(M * 4); b.rstd1 = take(M * 4);
      b.qkv = take(M * 3 * d * as);
      b.lse = take(seqs * heads * T * 4);
      b.att = take(M * d * as);
      b.x_mid = take(M * d * 4);
      b.ln2 = take(M * d * as); b.mean2 = take(M * 4); b.rstd2 = take(M * 4);
      b.fc1_pre = take(M * e->mlp * d * as);
      b.fc1_act = take(M * e->mlp * d * as);
      xs[i + 1] = take(M * d * 4);
    }
  };
  layers(e->depth, pl.Me, e->D, e->H, k, pl.enc_x, pl.enc);
  pl.enc_norm = take(pl.Me * e->D * as); pl.enc_mean = take(pl.Me * 4); pl.enc_rstd = take(pl.Me * 4);
  pl.xdec = take(pl.Me * e->Dd * as);
  layers(e->dd, pl.Md, e->Dd, e->Hd, dec_T, pl.dec_x, pl.dec);
  pl.dec_norm = take(std::max<int64_t>(pl.Mp, 1) * e->Dd * as);
  pl.dec_mean = take(std::max<int64_t>(pl.Mp, 1) * 4); pl.dec_rstd = take(std::max<int64_t>(pl.Mp, 1) * 4);
  pl.pred = take(std::max<int64_t>(pl.Mp, 1) * e->PO * 4);
  // backward scratch, shared by the decoder and encoder sweeps
  const int64_t R = std::max(pl.Me * e->D, pl.Md * e->Dd);
  pl.branch_a = take(R * as);
  pl.branch_b = take(R * as);
  pl.dpred = take(std::max<int64_t>(pl.Mp, 1) * e->PO * as);
  pl.d_decn = take(std::max<int64_t>(pl.Mp, 1) * e->Dd * as);
  pl.dres = take(R * 4);
  pl.dres_c = take(R * as);
  pl.d_ln = take(R * as);
  pl.d_att = take(R * as);
  pl.d_qkv = take(3 * R * as);
  pl.d_hidden = take((int64_t)e->mlp * R * as);
  pl.d_xdec = take(pl.Me * e->Dd * as);
  pl.dtok = take(pl.Me * e->D * as);
  const int maxd = std::max(e->D, e->Dd);
  pl.ln_partial_stride = (int64_t)2 * LN_BWD_MAX_BLOCKS * maxd * 4;  // one slot per LayerNorm of the backward pass: their
  pl.ln_partial = take(pl.ln_partial_stride * std::min(2 * (e->depth + e->dd) + 2, (int)PartialsTable::MAX));  // second stages run in one launch at the end
  pl.split_partial = take((int64_t)512 * maxd * 4);
  int64_t wg = 0;
  auto wgs = [&](int64_t M, int N, int K) { wg = std::max(wg, linear_wgrad_scratch_bytes(M, N, K)); };
  wgs(pl.Me, 3 * e->D, e->D); wgs(pl.Me, e->mlp * e->D, e->D); wgs(pl.Me, e->D, e->mlp * e->D); wgs(pl.Me, e->D, e->D);
  wgs(pl.Md, 3 * e->Dd, e->Dd); wgs(pl.Md, e->mlp * e->Dd, e->Dd); wgs(pl.Md, e->Dd, e->mlp * e->Dd); wgs(pl.Md, e->Dd, e->Dd);
  wgs(pl.Me, e->D, e->P); wgs(pl.Me, e->Dd, e->D); wgs(std::max<int64_t>(pl.Mp, 1), e->PO, e->Dd);
  auto wgp = [&](int64_t M, int d) {  // the paired launches of a block: fc2 + fc1, proj + qkv
    wg = std::max(wg, linear_wgrad_pair_scratch_bytes(M, d, e->mlp * d, e->mlp * d, d));
    wg = std::max(wg, linear_wgrad_pair_scratch_bytes(M, d, d, 3 * d, d));
  };
  wgp(pl.Me, e->D); wgp(pl.Md, e->Dd);
  pl.wgrad_scratch = take(wg);
  pl.loss_scratch = take(4096 * 4);
  pl.total = off;
  return pl;
}
static Plan make_plan(const mae_engine* e, int B, int k) { return make_plan_ex(e, B, k, B, e->L, e->L - k); }
// The encoder alone over every token of every image -- [cls | patches], or the patches alone (what an I-JEPA encoder sees) -- with a
// token-sized decoder stub: the I-JEPA target phase, the patch-only classifier and the frozen-encoder features.
static Plan make_encoder_plan(const mae_engine* e, int B, bool with_cls) { return make_plan_ex(e, B, with_cls ? e->L : e->L - 1, 1, 1, 1); }

// ---------------------------------------------------------------------------------------------------
// timers
// ---------------------------------------------------------------------------------------------------
struct TimerScope {
  mae_engine* e; int kind; hipStream_t s; hipEvent_t stop = nullptr;
  TimerScope(mae_engine* e_, int kind_, double flops, double bytes, hipStream_t s_) : e(e_), kind(kind_), s(s_) {
    if (!e->timers_on) return;
    TimerSlot& t = e->timers[kind];
    if (t.used == t.ev.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      t.ev.push_back({a, b});
    }
    (void)hipEventRecord(t.ev[t.used].first, s);
    stop = t.ev[t.used].second;
    t.used++;
    t.flops += flops;
    t.bytes += bytes;
  }
  ~TimerScope() { if (stop) (void)hipEventRecord(stop, s); }
};

#define RUN(kind, flops, bytes, expr)                      \
  do {                                                     \
    TimerScope _ts(e, kind, (double)(flops), (double)(bytes), s); \
    MAE_TRY(expr);                                         \
  } while (0)

// ---------------------------------------------------------------------------------------------------
// helpers bound to one call
// ---------------------------------------------------------------------------------------------------
struct Ctx {
  mae_engine* e;
  const float* params;
  const char* wcache;  // bf16 copies (null in fp32 mode)
  float* grads;
  char* ws;
  hipStream_t s;
  int act;
  int64_t as;
  void* const* ready = nullptr;  // hipEvent_t per gradient-ready point (entries may be null), or null
  bool fwd_only = false;         // no backward will follow (I-JEPA target encoder): the MLP saves no derivative
  // the frozen read-outs: -1 runs every block and the final norm; >= 0 runs blocks 0 .. last_block and returns before the norm, so
  // that x_mid + branch_b of that block is left for the caller
  int last_block = -1;
  // taps (the pooled features alone): right after block tap_layers[i] the feature kernel pools x_mid + branch_b into slice i of
  // tap_out (batch, tap_n, W); last_block = tap_layers[tap_n - 1]
  const int32_t* tap_layers = nullptr;
  int tap_n = 0, tap_with_cls = 1, tap_pool = MAE_POOL_CLS, tap_normalize = MAE_FEAT_NONE;
  float* tap_out = nullptr;
  const float* branch_scale = nullptr;  // drop path (classifier training only): (2 * depth, batch) per-image scales of the encoder's branches
  // row j of the table (row 2i: attention branch of encoder block i, 2i + 1: its MLP branch), or null without a table
  const float* scale_row(int j, int batch) const { return branch_scale ? branch_scale + (int64_t)j * batch : nullptr; }
  const float* P(int i) const { return params + e->params[i].offset; }
  float* Gp(int i) const { return grads + e->params[i].offset; }
  // GEMM operand view of weight i: (out, in) row-major in the activation dtype
  const void* W(int i) const {
    return act == MAE_BF16 ? (const void*)(wcache + 2 * e->params[i].offset) : (const void*)(params + e->params[i].offset);
  }
  // transposed (in, out) bf16 copy (bf16 mode only)
  const void* WT(int i) const { return wcache + 2 * (e->trainable_elems + e->params[i].t_off); }
  template <class T = void> T* buf(int64_t off) const { return reinterpret_cast<T*>(ws + off); }
};

// the one place a Ctx is built; `ready` / `fwd_only` / `last_block` / the taps are set by the few callers that need them
static Ctx make_ctx(mae_engine* e, const float* params, const void* wcache, float* grads, void* ws, void* stream) {
  return Ctx{e, params, (const char*)wcache, grads, (char*)ws, (hipStream_t)stream, e->act, (int64_t)dtype_size(e->act)};
}

// keep32 of a plan over every token of every image: tokens 0 .. L-1, or 1 .. L-1 without the class token
static int keep_every_token(const Ctx& c, const Plan& pl, bool with_cls) {
  return launch_iota_tokens(c.buf<int32_t>(pl.keep32), pl.B, pl.k, with_cls ? 0 : 1, c.s);
}

// algorithmic HBM bytes of one Linear launch: both operands, every output (the GELU epilogues write two) and the (M,N) side input
// of the RESID (fp32 residual) / MUL / DGELU (output-typed) epilogues
static double gemm_bytes(int64_t M, int N, int K, int64_t as, int64_t os, int mode = MAE_EPI_NONE) {
  const int64_t outs = (mode == MAE_EPI_GELU || mode == MAE_EPI_GELU_GRAD) ? 2 : 1;
  const int64_t side = mode == MAE_EPI_RESID ? 4 : (mode == MAE_EPI_MUL || mode == MAE_EPI_DGELU) ? os : 0;
  return (double)(M * K * as + (int64_t)N * K * as + M * N * (outs * os + side));
}

static int linear(const Ctx& c, const void* A, int wi, int bi, int64_t M, int N, int K, int mode, int out_dt, void* out, void* out2,
                  const void* aux) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  Epi ep; ep.mode = mode; ep.bias = bi >= 0 ? c.P(bi) : nullptr; ep.aux = aux; ep.out = out; ep.out2 = out2; ep.out_dt = out_dt;
  RUN(TK_LINEAR, 2.0 * M * N * K, gemm_bytes(M, N, K, c.as, (int64_t)dtype_size(out_dt), mode), launch_linear_fwd(A, c.W(wi), M, N, K, c.act, ep, s));
  return 0;
}

// dX[M,K] = dY[M,N] * W[N,K]
static int dgrad(const Ctx& c, const void* dY, int wi, int64_t M, int N, int K, int mode, void* out, const void* aux) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  Epi ep; ep.mode = mode; ep.aux = aux; ep.out = out; ep.out_dt = c.act;
  if (c.act == MAE_BF16) {
    RUN(TK_LINEAR, 2.0 * M * N * K, gemm_bytes(M, K, N, 2, 2, mode), launch_linear_fwd(dY, c.WT(wi), M, K, N, MAE_BF16, ep, s));
  } else {
    RUN(TK_LINEAR, 2.0 * M * N * K, gemm_bytes(M, K, N, 4, 4, mode), launch_linear_dgrad(dY, c.W(wi), M, N, K, MAE_F32, ep, s));
  }
  return 0;
}

static int wgrad(const Ctx& c, const Plan& pl, const void* dY, const void* A, int64_t M, int N, int K, int wi, int bi) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  RUN(TK_WGRAD, 2.0 * M * N * K, (double)(M * (N + K) * c.as + (int64_t)N * K * 4),
      launch_linear_wgrad(dY, A, M, N, K, c.act, c.Gp(wi), bi >= 0 ? c.Gp(bi) : nullptr, c.buf<>(pl.wgrad_scratch), s));
  return 0;
}

// two weight gradients over the same rows in one launch (k_gemm_tn.hip: launch_linear_wgrad_pair, which falls back to two
// launches under MAE_WGRAD_PAIR=0 or below its size threshold)
static int wgrad_pair(const Ctx& c, const Plan& pl, int64_t M, const void* dY0, const void* A0, int N0, int K0, int w0, int b0,
                      const void* dY1, const void* A1, int N1, int K1, int w1, int b1) {
  mae_engine* e = c.e;
  hipStream_t s = c.s;
  RUN(TK_WGRAD, 2.0 * M * ((double)N0 * K0 + (double)N1 * K1),
      (double)(M * (int64_t)(N0 + K0 + N1 + K1) * c.as + ((int64_t)N0 * K0 + (int64_t)N1 * K1) * 4),
      launch_linear_wgrad_pair(dY0, A0, N0, K0, c.Gp(w0), c.Gp(b0), dY1, A1, N1, K1, c.Gp(w1), c.Gp(b1), M, c.act, c.buf<>(pl.wgrad_scratch), s));
  return 0;
}

// y = LayerNorm(x [+ branch]) * gamma + beta over `rows` rows of width d (the rows row_map names, when given).  With a branch (in
// y's dtype) the sum x + branch is also written to x_sum (fp32): the fused residual add.
// Traffic per element: x in (4) + y out; the fused add also reads the branch and writes the sum (4).
// image_scale (drop path, optional): the branch of an image of T rows is multiplied by image_scale[image] in the add.
static int ln_fwd(const Ctx& c, const float* x, const void* branch, float* x_sum, const int32_t* row_map, const float* gamma,
                  const float* beta, float eps, int64_t rows, int d, int y_dt, void* y, float* mean, float* rstd,
                  const float* image_scale = nullptr, int T = 0) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int64_t ys = (int64_t)dtype_size(y_dt);
  RUN(TK_LN_FWD, 0, rows * d * (branch ? 8 + 2 * ys : 4 + ys),
      launch_layernorm_fwd(x, branch, x_sum, row_map, gamma, beta, eps, rows, d, y_dt, y, mean, rstd, s, image_scale, T));
  return 0;
}

// Backward of the LayerNorm with weight wi / bias bi for dy (activation dtype).  dx is written to (accumulate = 0) or added into
// (accumulate = 1) the residual gradient pl.dres, and pl.dres_c, its activation-dtype copy, is rewritten.  The dgamma / dbeta column
// sums go to the next partial-sum slot of this pass; their second stage is queued in e->ln_tab (flushed by reach_point / backward_end).
// Traffic per element: x in, dres in and out (12); dy in and dres_c out (two activation elements).
// copy_scale (drop path, optional): dres_c gets copy_scale[image] * dres, the gradient entering the branch that reads dres_c next.
static int ln_bwd(const Ctx& c, const Plan& pl, const void* dy, const float* x, const int32_t* row_map, int wi, int bi, const float* mean,
                  const float* rstd, int64_t rows, int d, int accumulate, const float* copy_scale = nullptr, int T = 0) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  float* slot = c.buf<float>(pl.ln_partial + (int64_t)(e->ln_tab.n % PartialsTable::MAX) * pl.ln_partial_stride);
  RUN(TK_LN_BWD, 0, rows * d * (12 + 2 * c.as),
      launch_layernorm_bwd(dy, c.act, x, row_map, c.P(wi), mean, rstd, rows, d, accumulate, c.buf<float>(pl.dres), c.buf<>(pl.dres_c),
                           c.Gp(wi), c.Gp(bi), slot, s, &e->ln_tab, copy_scale, T));
  return 0;
}

// One transformer block.  The residual adds are done by the LayerNorm kernels: LN1 first forms this block's input
// x_in = x_prev + prev_branch (the previous block's MLP output; none for the first block), LN2 forms x_mid = x_in + proj(att).
// The block's own MLP output is left in pl.branch_b for whoever normalises next.
// Drop path: scale_prev (Bn) scales the previous block's MLP branch in LN1's add, scale_att (Bn) this block's attention branch in LN2's.
static int block_forward(const Ctx& c, const Plan& pl, const BlockRefs& r, const LayerBufs& b, int64_t M, int d, int heads, int Bn, int T,
                         int64_t x_prev, bool add_prev, int64_t x_in, const float* scale_prev = nullptr, const float* scale_att = nullptr) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int hd = d / heads, hid = e->mlp * d;
  const float eps = 1e-6f;
  MAE_TRY(ln_fwd(c, c.buf<float>(add_prev ? x_prev : x_in), add_prev ? c.buf<>(pl.branch_b) : nullptr, add_prev ? c.buf<float>(x_in) : nullptr,
                 nullptr, c.P(r.ln1_w), c.P(r.ln1_b), eps, M, d, c.act, c.buf<>(b.ln1), c.buf<float>(b.mean1), c.buf<float>(b.rstd1),
                 add_prev ? scale_prev : nullptr, T));
  MAE_TRY(linear(c, c.buf<>(b.ln1), r.qkv_w, r.qkv_b, M, 3 * d, d, MAE_EPI_NONE, c.act, c.buf<>(b.qkv), nullptr, nullptr));
  RUN(TK_ATTN_FWD, 4.0 * Bn * heads * (double)T * T * hd, M * 4 * d * c.as, launch_attention_fwd(c.buf<>(b.qkv), Bn, T, heads, hd, c.act, c.buf<>(b.att), c.buf<float>(b.lse), s));
  MAE_TRY(linear(c, c.buf<>(b.att), r.proj_w, r.proj_b, M, d, d, MAE_EPI_NONE, c.act, c.buf<>(pl.branch_a), nullptr, nullptr));
  MAE_TRY(ln_fwd(c, c.buf<float>(x_in), c.buf<>(pl.branch_a), c.buf<float>(b.x_mid), nullptr, c.P(r.ln2_w), c.P(r.ln2_b), eps, M, d, c.act,
                 c.buf<>(b.ln2), c.buf<float>(b.mean2), c.buf<float>(b.rstd2), scale_att, T));
  if (c.fwd_only)
    MAE_TRY(linear(c, c.buf<>(b.ln2), r.fc1_w, r.fc1_b, M, hid, d, MAE_EPI_GELU_ACT, c.act, c.buf<>(b.fc1_act), nullptr, nullptr));
  else
    MAE_TRY(linear(c, c.buf<>(b.ln2), r.fc1_w, r.fc1_b, M, hid, d, MAE_EPI_GELU_GRAD, c.act, c.buf<>(b.fc1_pre), c.buf<>(b.fc1_act), nullptr));  // fc1_pre holds gelu'(pre)
  MAE_TRY(linear(c, c.buf<>(b.fc1_act), r.fc2_w, r.fc2_b, M, d, hid, MAE_EPI_NONE, c.act, c.buf<>(pl.branch_b), nullptr, nullptr));
  return 0;
}

// in: dres (fp32) / dres_c (act copy) = gradient w.r.t. the block output; out: same buffers = gradient w.r.t. the block input.
// Each branch's two weight gradients go out as ONE launch, placed where both of their dY operands exist and before the
// LayerNorm backward that rewrites dres_c (fc2 / proj read it).
// Drop path: whoever writes dres_c scales it for the branch that reads it next, so the copy arrives here scaled for this block's MLP
// branch; LN2's backward scales its copy by scale_att (Bn) for the attention branch, LN1's by scale_prev (Bn) for the MLP branch of the
// block below (null for the first block, whose copy nobody reads as a branch gradient).
static int block_backward(const Ctx& c, const Plan& pl, const BlockRefs& r, const LayerBufs& b, int64_t M, int d, int heads, int Bn, int T,
                          int64_t x_in, const float* scale_prev = nullptr, const float* scale_att = nullptr) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int hd = d / heads, hid = e->mlp * d;
  void* dres_c = c.buf<>(pl.dres_c);
  // MLP branch
  MAE_TRY(dgrad(c, dres_c, r.fc2_w, M, d, hid, MAE_EPI_MUL, c.buf<>(pl.d_hidden), c.buf<>(b.fc1_pre)));
  MAE_TRY(wgrad_pair(c, pl, M, dres_c, c.buf<>(b.fc1_act), d, hid, r.fc2_w, r.fc2_b, c.buf<>(pl.d_hidden), c.buf<>(b.ln2), hid, d, r.fc1_w, r.fc1_b));
  MAE_TRY(dgrad(c, c.buf<>(pl.d_hidden), r.fc1_w, M, hid, d, MAE_EPI_NONE, c.buf<>(pl.d_ln), nullptr));
  MAE_TRY(ln_bwd(c, pl, c.buf<>(pl.d_ln), c.buf<float>(b.x_mid), nullptr, r.ln2_w, r.ln2_b, c.buf<float>(b.mean2), c.buf<float>(b.rstd2), M, d, 1, scale_att, T));
  // attention branch
  MAE_TRY(dgrad(c, dres_c, r.proj_w, M, d, d, MAE_EPI_NONE, c.buf<>(pl.d_att), nullptr));
  RUN(TK_ATTN_BWD, 10.0 * Bn * heads * (double)T * T * hd, M * 9 * d * c.as, launch_attention_bwd(c.buf<>(b.qkv), c.buf<>(b.att), c.buf<>(pl.d_att), c.buf<float>(b.lse), Bn, T, heads, hd, c.act, c.buf<>(pl.d_qkv), s));
  MAE_TRY(wgrad_pair(c, pl, M, dres_c, c.buf<>(b.att), d, d, r.proj_w, r.proj_b, c.buf<>(pl.d_qkv), c.buf<>(b.ln1), 3 * d, d, r.qkv_w, r.qkv_b));
  MAE_TRY(dgrad(c, c.buf<>(pl.d_qkv), r.qkv_w, M, 3 * d, d, MAE_EPI_NONE, c.buf<>(pl.d_ln), nullptr));
  MAE_TRY(ln_bwd(c, pl, c.buf<>(pl.d_ln), c.buf<float>(x_in), nullptr, r.ln1_w, r.ln1_b, c.buf<float>(b.mean1), c.buf<float>(b.rstd1), M, d, 1, scale_prev, T));
  return 0;
}

static bool batch_in_bound(const mae_engine* e, int B) {  // the engine's batch bound: B * L * widest layer < 2^40
  return (int64_t)B * e->L * std::max(3 * e->D, e->mlp * std::max(e->D, e->Dd)) < (1ll << 40);
}

// The rules every engine call shares: engine, arena and workspace present and aligned, the weight cache of a bf16 engine, the
// batch bound.  Each entry point adds its own workspace plan and token-count rules.
static int check_common(const mae_engine* e, const void* params, const void* wcache, int B, const void* ws, const char* who) {
  MAE_REQUIRE(e, "%s: null engine", who);
  MAE_REQUIRE(params && ws, "%s: null params/workspace", who);
  MAE_REQUIRE(e->act == MAE_F32 || wcache, "%s: bf16 engine needs the weight cache", who);
  MAE_REQUIRE(batch_in_bound(e, B), "%s: batch too large", who);
  MAE_REQUIRE(((uintptr_t)ws & 255) == 0 && ((uintptr_t)params & 15) == 0, "%s: workspace must be 256-byte aligned, params 16-byte", who);
  return 0;
}

static int check_call(const mae_engine* e, const void* params, const void* wcache, int B, int k, const void* ws, int64_t ws_bytes,
                      Plan* pl, const char* who) {
  MAE_TRY(check_common(e, params, wcache, B, ws, who));
  MAE_REQUIRE(B > 0 && k >= 1 && k <= e->L, "%s: batch %d / num_keep %d out of range (L = %d)", who, B, k, e->L);
  *pl = make_plan(e, B, k);
  MAE_REQUIRE(ws_bytes >= pl->total, "%s: workspace too small (%lld < %lld bytes)", who, (long long)ws_bytes, (long long)pl->total);
  return 0;
}

static int check_image_dtype(int dt, const char* who) {
  MAE_REQUIRE(dt == MAE_F32 || dt == MAE_U8, "%s: image_dtype must be MAE_F32 or MAE_U8 (got %d)", who, dt);
  return 0;
}

// Tap `slot` of the call: block i has just run, so pl.enc[i].x_mid and pl.branch_b hold its residual stream until the next block's fc2
// rewrites the branch.  The encoder's final norm, as for the last block.  Bytes: the pooled rows read, the slice written.
static int tap_block(const Ctx& c, const Plan& pl, int i, int slot) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int T = pl.k, W = features_tap_width(c.tap_pool, e->D);
  const int lo = c.tap_pool == MAE_POOL_MEAN_PATCHES && c.tap_with_cls ? 1 : 0, hi = c.tap_pool == MAE_POOL_CLS ? 1 : T;
  RUN(TK_LN_FWD, 0, (double)pl.B * (hi - lo) * e->D * (4 + c.as) + (double)pl.B * W * 4,
      launch_features_tap(c.buf<float>(pl.enc[i].x_mid), c.buf<>(pl.branch_b), e->act, c.P(e->i_norm_w), c.P(e->i_norm_b), 1e-6f, pl.B, T, e->D,
                          c.tap_with_cls, c.tap_pool, c.tap_normalize, c.tap_out + (int64_t)slot * W, (int64_t)c.tap_n * W, s));
  return 0;
}

static int forward_encoder_impl(const Ctx& c, const Plan& pl, const void* images, int img_dt, float* x_encoded_out) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int32_t* keep32 = c.buf<int32_t>(pl.keep32);
  // bytes read: uint8 images go whole through LDS (every pixel byte is fetched once), float images give up their kept patches only
  const int64_t gather_read = img_dt == MAE_U8 ? (int64_t)pl.B * e->C * e->img * e->img : pl.Me * e->P * 4;
  RUN(TK_DATA, 0, gather_read + pl.Me * e->P * c.as, launch_gather_patches(images, img_dt, keep32, pl.B, pl.k, e->C, e->img, e->p, c.act, c.buf<>(pl.patchA), s));
  MAE_TRY(linear(c, c.buf<>(pl.patchA), e->i_patch_w, e->i_patch_b, pl.Me, e->D, e->P, MAE_EPI_NONE, MAE_F32, c.buf<>(pl.enc_x[0]), nullptr, nullptr));
  RUN(TK_DATA, 0, pl.Me * e->D * 12, launch_assemble_visible(c.buf<float>(pl.enc_x[0]), keep32, c.P(e->i_cls), c.P(e->i_pos), pl.Me, e->D, s));
  const int blocks = c.last_block >= 0 ? c.last_block + 1 : e->depth;
  for (int i = 0, slot = 0; i < blocks; ++i) {
    MAE_TRY(block_forward(c, pl, e->enc[i], pl.enc[i], pl.Me, e->D, e->H, pl.B, pl.k, i ? pl.enc[i - 1].x_mid : 0, i > 0, pl.enc_x[i],
                          i ? c.scale_row(2 * i - 1, pl.B) : nullptr, c.scale_row(2 * i, pl.B)));
    if (slot < c.tap_n && c.tap_layers[slot] == i) MAE_TRY(tap_block(c, pl, i, slot++));
  }
  if (c.last_block >= 0) return 0;
  MAE_TRY(ln_fwd(c, c.buf<float>(pl.enc[e->depth - 1].x_mid), c.buf<>(pl.branch_b), c.buf<float>(pl.enc_x[e->depth]), nullptr, c.P(e->i_norm_w),
                 c.P(e->i_norm_b), 1e-6f, pl.Me, e->D, c.act, c.buf<>(pl.enc_norm), c.buf<float>(pl.enc_mean), c.buf<float>(pl.enc_rstd),
                 c.scale_row(2 * e->depth - 1, pl.B), pl.k));
  if (x_encoded_out) {
    if (c.act == MAE_F32) MAE_HIP(hipMemcpyAsync(x_encoded_out, c.buf<>(pl.enc_norm), (size_t)pl.Me * e->D * 4, hipMemcpyDeviceToDevice, s));
    else  // a second pass over the residual sum just formed writes the fp32 rows
      MAE_TRY(ln_fwd(c, c.buf<float>(pl.enc_x[e->depth]), nullptr, nullptr, nullptr, c.P(e->i_norm_w), c.P(e->i_norm_b), 1e-6f, pl.Me, e->D, MAE_F32,
                     x_encoded_out, c.buf<float>(pl.enc_mean), c.buf<float>(pl.enc_rstd)));
  }
  return 0;
}

// I-JEPA predictor input (no counterpart in the reference; spec in DESIGN.md): per image nblk sequences
// [k context tokens | m mask tokens of target block i], position rows gathered by token id
struct JepaSeq {
  const int32_t* ctx32;  // (B, k) context token ids
  const int32_t* tgt32;  // (B, nblk, m) target token ids
  int nblk;
};

// needs keep32 / mask32 already in the workspace (MAE) or the token lists of `jp` (I-JEPA)
static int forward_decoder_impl(const Ctx& c, const Plan& pl, float* x_pred_out, const JepaSeq* jp = nullptr) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  MAE_REQUIRE(pl.m > 0, "forward_decoder: nothing is masked (num_keep == sequence_length)");
  MAE_TRY(linear(c, c.buf<>(pl.enc_norm), e->i_de_w, e->i_de_b, pl.Me, e->Dd, e->D, MAE_EPI_NONE, c.act, c.buf<>(pl.xdec), nullptr, nullptr));
  if (jp) {
    MAE_TRY(launch_build_tail_row_map(pl.dec_B, pl.dec_T, pl.m, c.buf<int32_t>(pl.pred_rows), s));
    RUN(TK_DATA, 0, pl.Md * e->Dd * 4 + pl.Me * e->Dd * c.as, launch_predictor_assemble(c.buf<>(pl.xdec), c.act, jp->ctx32, jp->tgt32, c.P(e->i_dec_mask), c.P(e->i_dec_pos), pl.B, pl.k, jp->nblk, pl.m, e->L, e->Dd, c.buf<float>(pl.dec_x[0]), s));
  } else {
    MAE_TRY(launch_build_inverse(c.buf<int32_t>(pl.keep32), pl.B, pl.k, e->L, c.buf<int32_t>(pl.inv), s));
    MAE_TRY(launch_build_row_map(c.buf<int32_t>(pl.mask32), pl.B, pl.m, e->L, c.buf<int32_t>(pl.pred_rows), s));
    RUN(TK_DATA, 0, pl.Md * e->Dd * 4 + pl.Me * e->Dd * c.as, launch_decoder_assemble(c.buf<>(pl.xdec), c.act, c.buf<int32_t>(pl.inv), c.P(e->i_dec_mask), c.P(e->i_dec_pos), pl.B, pl.k, e->L, e->Dd, c.buf<float>(pl.dec_x[0]), s));
  }
  for (int i = 0; i < e->dd; ++i)
    MAE_TRY(block_forward(c, pl, e->dec[i], pl.dec[i], pl.Md, e->Dd, e->Hd, pl.dec_B, pl.dec_T, i ? pl.dec[i - 1].x_mid : 0, i > 0, pl.dec_x[i]));
  // decoder_norm on the masked rows only; the residual add of the last MLP branch is done for exactly those rows
  MAE_TRY(ln_fwd(c, c.buf<float>(pl.dec[e->dd - 1].x_mid), c.buf<>(pl.branch_b), c.buf<float>(pl.dec_x[e->dd]), c.buf<int32_t>(pl.pred_rows),
                 c.P(e->i_dn_w), c.P(e->i_dn_b), 1e-6f, pl.Mp, e->Dd, c.act, c.buf<>(pl.dec_norm), c.buf<float>(pl.dec_mean), c.buf<float>(pl.dec_rstd)));
  MAE_TRY(linear(c, c.buf<>(pl.dec_norm), e->i_pred_w, e->i_pred_b, pl.Mp, e->PO, e->Dd, MAE_EPI_NONE, MAE_F32, x_pred_out ? (void*)x_pred_out : c.buf<>(pl.pred), nullptr, nullptr));
  return 0;
}

// Gradient-ready points (data-parallel overlap): point 0 = the whole decoder range of the gradient arena is final, point
// i (1 .. depth-1) = encoder block depth-i and everything behind it, point depth = everything.  Reaching a point that the
// caller gave an event for first retires what was deferred (the LayerNorm dgamma / dbeta second stages).
static int reach_point(const Ctx& c, int j) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  if (!c.ready || !c.ready[j]) return 0;
  if (e->ln_tab.n > 0) {
    RUN(TK_LN_BWD, 0, 0, launch_sum_partials_many(e->ln_tab, s));
    e->ln_tab.n = 0;  // slots are reused in stream order behind the reduction just enqueued
  }
  MAE_HIP(hipEventRecord((hipEvent_t)c.ready[j], s));
  return 0;
}

static void backward_begin(const Ctx& c) { c.e->ln_tab.n = 0; }
static int backward_end(const Ctx& c) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  if (e->ln_tab.n > 0) RUN(TK_LN_BWD, 0, 0, launch_sum_partials_many(e->ln_tab, s));  // dgamma / dbeta of every LayerNorm not yet retired: one launch
  e->ln_tab.n = 0;
  return 0;
}

// Decoder half: dpred (act dtype) must already sit in the workspace; leaves d(x_encoded) (act dtype) in pl.d_ln and
// every decoder gradient in its arena range [offset(decoder.mask_token), trainable_elems).
static int backward_decoder_impl(const Ctx& c, const Plan& pl, const JepaSeq* jp = nullptr) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  float* dres = c.buf<float>(pl.dres);
  // prediction head
  MAE_TRY(wgrad(c, pl, c.buf<>(pl.dpred), c.buf<>(pl.dec_norm), pl.Mp, e->PO, e->Dd, e->i_pred_w, e->i_pred_b));
  MAE_TRY(dgrad(c, c.buf<>(pl.dpred), e->i_pred_w, pl.Mp, e->PO, e->Dd, MAE_EPI_NONE, c.buf<>(pl.d_decn), nullptr));
  // decoder_norm over the masked rows only: every other row of the residual gradient is zero
  RUN(TK_DATA, 0, (pl.Md - pl.Mp) * e->Dd * (4 + c.as), launch_zero_unpredicted_rows(jp ? nullptr : c.buf<int32_t>(pl.inv), pl.Md, pl.dec_T, pl.m, e->Dd, c.act, dres, c.buf<>(pl.dres_c), s));
  MAE_TRY(ln_bwd(c, pl, c.buf<>(pl.d_decn), c.buf<float>(pl.dec_x[e->dd]), c.buf<int32_t>(pl.pred_rows), e->i_dn_w, e->i_dn_b, c.buf<float>(pl.dec_mean),
                 c.buf<float>(pl.dec_rstd), pl.Mp, e->Dd, 0));
  for (int i = e->dd - 1; i >= 0; --i)
    MAE_TRY(block_backward(c, pl, e->dec[i], pl.dec[i], pl.Md, e->Dd, e->Hd, pl.dec_B, pl.dec_T, pl.dec_x[i]));
  if (jp)
    RUN(TK_DATA, 0, pl.Md * e->Dd * 4 + pl.Me * e->Dd * c.as, launch_predictor_assemble_bwd(dres, pl.B, pl.k, jp->nblk, pl.m, e->Dd, c.act, c.buf<>(pl.d_xdec), c.Gp(e->i_dec_mask), c.buf<float>(pl.split_partial), s));
  else
    RUN(TK_DATA, 0, pl.Md * e->Dd * 4 + pl.Me * e->Dd * c.as, launch_decoder_assemble_bwd(dres, c.buf<int32_t>(pl.inv), pl.B, pl.k, e->L, e->Dd, c.act, c.buf<>(pl.d_xdec), c.Gp(e->i_dec_mask), c.buf<float>(pl.split_partial), s));
  // decoder_embed
  MAE_TRY(wgrad(c, pl, c.buf<>(pl.d_xdec), c.buf<>(pl.enc_norm), pl.Me, e->Dd, e->D, e->i_de_w, e->i_de_b));
  MAE_TRY(dgrad(c, c.buf<>(pl.d_xdec), e->i_de_w, pl.Me, e->Dd, e->D, MAE_EPI_NONE, c.buf<>(pl.d_ln), nullptr));
  return reach_point(c, 0);
}

// Encoder half: d(x_encoded) (act dtype) sits in pl.d_ln; writes the arena range [0, offset(decoder.mask_token)).
static int backward_encoder_impl(const Ctx& c, const Plan& pl) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  MAE_TRY(ln_bwd(c, pl, c.buf<>(pl.d_ln), c.buf<float>(pl.enc_x[e->depth]), nullptr, e->i_norm_w, e->i_norm_b, c.buf<float>(pl.enc_mean),
                 c.buf<float>(pl.enc_rstd), pl.Me, e->D, 0));
  for (int i = e->depth - 1; i >= 0; --i) {
    MAE_TRY(block_backward(c, pl, e->enc[i], pl.enc[i], pl.Me, e->D, e->H, pl.B, pl.k, pl.enc_x[i]));
    if (i > 0) MAE_TRY(reach_point(c, e->depth - i));
  }
  // token assembly and patch projection
  RUN(TK_DATA, 0, pl.Me * e->D * (4 + c.as), launch_visible_grad_split(c.buf<float>(pl.dres), c.buf<int32_t>(pl.keep32), pl.Me, e->D, c.act, c.buf<>(pl.dtok), c.Gp(e->i_cls), c.buf<float>(pl.split_partial), s));
  MAE_TRY(wgrad(c, pl, c.buf<>(pl.dtok), c.buf<>(pl.patchA), pl.Me, e->D, e->P, e->i_patch_w, e->i_patch_b));
  return 0;
}

static int backward_impl(const Ctx& c, const Plan& pl, const float* d_x_encoded_extra = nullptr, const JepaSeq* jp = nullptr) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  backward_begin(c);
  MAE_TRY(backward_decoder_impl(c, pl, jp));
  if (d_x_encoded_extra) MAE_TRY(launch_add_into(d_x_encoded_extra, c.buf<>(pl.d_ln), c.act, pl.Me * e->D, s));
  MAE_TRY(backward_encoder_impl(c, pl));
  MAE_TRY(backward_end(c));
  if (c.ready && c.ready[e->depth]) MAE_HIP(hipEventRecord((hipEvent_t)c.ready[e->depth], s));
  return 0;
}

}  // namespace mae

// =====================================================================================================
// C ABI
// =====================================================================================================
extern "C" const char* mae_last_error(void) { return mae::g_err; }
extern "C" int mae_abi_version(void) { return MAE_ABI_VERSION; }

extern "C" int mae_engine_create(const mae_config_t* cfg, mae_engine_t** out) {
  MAE_REQUIRE(cfg && out, "mae_engine_create: null argument");
  MAE_REQUIRE(cfg->image_size > 0 && cfg->patch_size > 0 && cfg->image_size % cfg->patch_size == 0,
              "image_size %d must be a positive multiple of patch_size %d", cfg->image_size, cfg->patch_size);
  MAE_REQUIRE(cfg->in_chans > 0 && cfg->embed_dim > 0 && cfg->depth > 0 && cfg->decoder_embed_dim > 0 && cfg->decoder_depth > 0,
              "mae_engine_create: non-positive model dimension");
  MAE_REQUIRE(cfg->num_heads > 0 && cfg->embed_dim % cfg->num_heads == 0, "dim should be divisible by num_heads (%d %% %d)", cfg->embed_dim, cfg->num_heads);
  MAE_REQUIRE(cfg->decoder_num_heads > 0 && cfg->decoder_embed_dim % cfg->decoder_num_heads == 0,
              "decoder dim should be divisible by decoder_num_heads (%d %% %d)", cfg->decoder_embed_dim, cfg->decoder_num_heads);
  MAE_REQUIRE(cfg->embed_dim % 4 == 0 && cfg->decoder_embed_dim % 4 == 0 && cfg->embed_dim <= 1024 && cfg->decoder_embed_dim <= 1024,
              "embed dims must be multiples of 4 and <= 1024");
  MAE_REQUIRE(cfg->act_dtype == MAE_F32 || cfg->act_dtype == MAE_BF16, "act_dtype must be MAE_F32 or MAE_BF16");
  for (int hd : {cfg->embed_dim / cfg->num_heads, cfg->decoder_embed_dim / cfg->decoder_num_heads})
    MAE_REQUIRE(hd == 16 || hd == 24 || hd == 32 || hd == 48 || hd == 64,
                "head dim %d is not supported by the attention kernels (16, 24, 32, 48 or 64): choose num_heads accordingly", hd);
  const int P = cfg->patch_size * cfg->patch_size * cfg->in_chans;
  MAE_REQUIRE(P % 4 == 0, "patch_size^2 * in_chans must be a multiple of 4");
  MAE_REQUIRE(cfg->pred_dim >= 0 && cfg->pred_dim % 4 == 0, "pred_dim must be 0 (pixels) or a multiple of 4");
  MAE_REQUIRE(cfg->norm_pix_loss == 0 || cfg->pred_dim == 0,
              "norm_pix_loss needs pixel targets: it cannot be combined with pred_dim = %d (the I-JEPA engine predicts latents)", cfg->pred_dim);
  mae_engine* e = new mae_engine();
  e->cfg = *cfg;
  e->act = cfg->act_dtype;
  e->D = cfg->embed_dim; e->depth = cfg->depth; e->H = cfg->num_heads;
  e->Dd = cfg->decoder_embed_dim; e->dd = cfg->decoder_depth; e->Hd = cfg->decoder_num_heads;
  e->C = cfg->in_chans; e->img = cfg->image_size; e->p = cfg->patch_size;
  e->G = e->img / e->p; e->L = e->G * e->G + 1; e->P = P;
  e->mlp = cfg->mlp_ratio > 0 ? cfg->mlp_ratio : 4;
  e->PO = cfg->pred_dim > 0 ? cfg->pred_dim : P;
  const int T = MAE_PARAM_TRAINABLE, M = MAE_PARAM_TRAINABLE | MAE_PARAM_MATRIX;
  // state_dict order
  e->i_enc_mask = add_param(e, "encoder.mask_token", {1, 1, e->D}, MAE_PARAM_UNUSED);
  e->i_cls = add_param(e, "encoder.vit.cls_token", {1, 1, e->D}, T);
  e->i_pos = add_param(e, "encoder.vit.pos_embed", {1, e->L, e->D}, MAE_PARAM_FROZEN);
  e->i_patch_w = add_param(e, "encoder.vit.patch_embed.proj.weight", {e->D, e->C, e->p, e->p}, M);
  e->i_patch_b = add_param(e, "encoder.vit.patch_embed.proj.bias", {e->D}, T);
  for (int i = 0; i < e->depth; ++i) e->enc.push_back(add_block(e, "encoder.vit.blocks." + std::to_string(i), e->D, e->mlp));
  e->i_norm_w = add_param(e, "encoder.vit.norm.weight", {e->D}, T);
  e->i_norm_b = add_param(e, "encoder.vit.norm.bias", {e->D}, T);
  e->i_dec_mask = add_param(e, "decoder.mask_token", {1, 1, e->Dd}, T);
  e->i_dec_pos = add_param(e, "decoder.decoder_pos_embed", {1, e->L, e->Dd}, MAE_PARAM_FROZEN);
  e->i_de_w = add_param(e, "decoder.decoder_embed.weight", {e->Dd, e->D}, M);
  e->i_de_b = add_param(e, "decoder.decoder_embed.bias", {e->Dd}, T);
  for (int i = 0; i < e->dd; ++i) e->dec.push_back(add_block(e, "decoder.decoder_blocks." + std::to_string(i), e->Dd, e->mlp));
  e->i_dn_w = add_param(e, "decoder.decoder_norm.weight", {e->Dd}, T);
  e->i_dn_b = add_param(e, "decoder.decoder_norm.bias", {e->Dd}, T);
  e->i_pred_w = add_param(e, "decoder.decoder_pred.weight", {e->PO, e->Dd}, M);
  e->i_pred_b = add_param(e, "decoder.decoder_pred.bias", {e->PO}, T);
  // arena: trainable-on-path first, then frozen / unused; 64-element alignment
  int64_t off = 0, toff = 0;
  for (auto& pi : e->params)
    if (pi.flags & MAE_PARAM_TRAINABLE) {
      pi.offset = off; off += round_up(pi.numel, 64);
      if (pi.flags & MAE_PARAM_MATRIX) { pi.t_off = toff; toff += round_up(pi.numel, 64); }
    }
  e->trainable_elems = off;
  for (auto& pi : e->params)
    if (!(pi.flags & MAE_PARAM_TRAINABLE)) { pi.offset = off; off += round_up(pi.numel, 64); }
  e->arena_elems = off;
  e->trans_elems = toff;
  *out = e;
  return 0;
}

extern "C" void mae_engine_destroy(mae_engine_t* e) {
  if (!e) return;
  for (auto& t : e->timers)
    for (auto& pr : t.ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  delete e;
}

extern "C" int64_t mae_engine_num_params(const mae_engine_t* e) { return e ? (int64_t)e->params.size() : 0; }
extern "C" int64_t mae_engine_arena_elems(const mae_engine_t* e) { return e ? e->arena_elems : 0; }
extern "C" int64_t mae_engine_trainable_elems(const mae_engine_t* e) { return e ? e->trainable_elems : 0; }

extern "C" int mae_engine_param_info(const mae_engine_t* e, int64_t index, const char** name, int64_t* offset, int64_t* numel,
                                     int32_t* ndim, int64_t shape[4], int32_t* flags) {
  MAE_REQUIRE(e && index >= 0 && index < (int64_t)e->params.size(), "mae_engine_param_info: index out of range");
  const ParamInfo& pi = e->params[index];
  if (name) *name = pi.name.c_str();
  if (offset) *offset = pi.offset;
  if (numel) *numel = pi.numel;
  if (ndim) *ndim = pi.ndim;
  if (shape) for (int i = 0; i < 4; ++i) shape[i] = pi.shape[i];
  if (flags) *flags = pi.flags;
  return 0;
}

extern "C" int64_t mae_engine_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_keep) {
  if (!e || batch <= 0 || num_keep < 1 || num_keep > e->L) return -1;
  return make_plan(e, batch, num_keep).total;
}

extern "C" int64_t mae_engine_wcache_bytes(const mae_engine_t* e) {
  if (!e || e->act != MAE_BF16) return 256;
  return round_up(2 * (e->trainable_elems + e->trans_elems), 256);
}

// transposed bf16 copies of the matrices that lie inside the arena range [lo, hi)
static int refresh_transposed(mae_engine* e, const float* params, void* wcache, hipStream_t s, int64_t lo = 0, int64_t hi = INT64_MAX) {
  bf16* tbase = reinterpret_cast<bf16*>(wcache) + e->trainable_elems;
  TransposeTable tab;
  auto flush = [&]() -> int {
    if (tab.n == 0) return 0;
    tab.total_tiles = tab.tile_begin[tab.n];
    const int r = launch_transpose_many(params, tbase, tab, s);
    tab.n = 0;
    return r;
  };
  tab.tile_begin[0] = 0;
  for (const auto& pi : e->params) {
    if (!(pi.flags & MAE_PARAM_MATRIX) || pi.t_off < 0 || pi.offset < lo || pi.offset + pi.numel > hi) continue;
    const int rows = (int)pi.shape[0], cols = (int)(pi.numel / pi.shape[0]);
    const int i = tab.n++;
    tab.src_off[i] = pi.offset; tab.dst_off[i] = pi.t_off; tab.rows[i] = rows; tab.cols[i] = cols;
    tab.tile_begin[i + 1] = tab.tile_begin[i] + (int)(cdiv(rows, TransposeTable::TILE) * cdiv(cols, TransposeTable::TILE));
    if (tab.n == TransposeTable::MAX) { MAE_TRY(flush()); tab.tile_begin[0] = 0; }
  }
  return flush();
}

extern "C" int mae_engine_refresh_weights(mae_engine_t* e, const float* params, void* wcache, void* stream) {
  MAE_REQUIRE(e && params, "mae_engine_refresh_weights: null argument");
  if (e->act != MAE_BF16) return 0;
  MAE_REQUIRE(wcache, "mae_engine_refresh_weights: null weight cache");
  hipStream_t s = (hipStream_t)stream;
  MAE_TRY(launch_f32_to_bf16(params, reinterpret_cast<bf16*>(wcache), e->trainable_elems, s));
  return refresh_transposed(e, params, wcache, s);
}

extern "C" int mae_engine_forward_encoder(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                                          int32_t image_dtype, const int64_t* idx_keep, int32_t batch, int32_t num_keep,
                                          void* workspace, int64_t workspace_bytes, float* x_encoded, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_forward_encoder"));
  MAE_REQUIRE(images && idx_keep, "mae_engine_forward_encoder: null images/idx_keep");
  MAE_TRY(check_image_dtype(image_dtype, "mae_engine_forward_encoder"));
  Ctx c = make_ctx(e, params, wcache, nullptr, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_idx_to_i32(idx_keep, c.buf<int32_t>(pl.keep32), pl.Me, s));
  return forward_encoder_impl(c, pl, images, image_dtype, x_encoded);
}

extern "C" int mae_engine_forward_decoder(mae_engine_t* e, const float* params, const void* wcache, const float* x_encoded,
                                          const int64_t* idx_keep, const int64_t* idx_mask, int32_t batch, int32_t num_keep,
                                          int32_t num_mask, void* workspace, int64_t workspace_bytes, float* x_pred, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_forward_decoder"));
  MAE_REQUIRE(idx_keep && idx_mask, "mae_engine_forward_decoder: null indices");
  MAE_REQUIRE(num_mask == pl.m, "mae_engine_forward_decoder: num_keep + num_mask must equal the sequence length (%d + %d != %d)", num_keep, num_mask, e->L);
  Ctx c = make_ctx(e, params, wcache, nullptr, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_idx_to_i32(idx_keep, c.buf<int32_t>(pl.keep32), pl.Me, s));
  MAE_TRY(launch_idx_to_i32(idx_mask, c.buf<int32_t>(pl.mask32), pl.Mp, s));
  if (x_encoded) MAE_TRY(launch_cast(x_encoded, MAE_F32, c.buf<>(pl.enc_norm), e->act, pl.Me * e->D, s));
  return forward_decoder_impl(c, pl, x_pred);
}

// MAEReconstructor.reconstruct_batch (scripts/evaluation/visualize_reconstruction.py:127-168): the two forwards above, then the compose
extern "C" int mae_engine_reconstruct(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                      const int64_t* idx_keep, const int64_t* idx_mask, int32_t batch, int32_t num_keep, int32_t num_mask,
                                      float fill, int32_t out_dtype, void* workspace, int64_t workspace_bytes, float* x_pred, void* recon,
                                      void* masked, float* stats, void* scratch, int64_t scratch_bytes, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_reconstruct"));
  MAE_REQUIRE(images && idx_keep && idx_mask, "mae_engine_reconstruct: null images/indices");
  MAE_TRY(check_image_dtype(image_dtype, "mae_engine_reconstruct"));
  MAE_REQUIRE(e->PO == e->P, "mae_engine_reconstruct: the engine predicts latents (pred_dim = %d), not pixels", e->PO);
  MAE_REQUIRE(num_mask == pl.m && pl.m > 0, "mae_engine_reconstruct: num_keep + num_mask must equal the sequence length (%d + %d != %d)", num_keep, num_mask, e->L);
  Ctx c = make_ctx(e, params, wcache, nullptr, workspace, stream);
  hipStream_t s = c.s;
  float* pred = x_pred ? x_pred : c.buf<float>(pl.pred);
  // norm_pix_loss: the decoder predicts in normalised space; the compose reads a de-normalised copy kept in the workspace's slot
  float* pixels = e->cfg.norm_pix_loss ? c.buf<float>(pl.pred) : pred;
  MAE_TRY(check_reconstruct_compose(images, image_dtype, pred, idx_mask, batch, e->C, e->img, e->p, num_mask, out_dtype, recon, masked, stats,
                                    scratch, scratch_bytes));
  if (pixels != pred)
    MAE_TRY(check_reconstruct_compose(images, image_dtype, pixels, idx_mask, batch, e->C, e->img, e->p, num_mask, out_dtype, recon, masked, stats,
                                      scratch, scratch_bytes));
  MAE_TRY(launch_idx_to_i32(idx_keep, c.buf<int32_t>(pl.keep32), pl.Me, s));
  MAE_TRY(launch_idx_to_i32(idx_mask, c.buf<int32_t>(pl.mask32), pl.Mp, s));
  MAE_TRY(forward_encoder_impl(c, pl, images, image_dtype, nullptr));
  MAE_TRY(forward_decoder_impl(c, pl, pred));
  if (e->cfg.norm_pix_loss)
    RUN(TK_DATA, 0, pl.Mp * e->P * (8 + (image_dtype == MAE_U8 ? 1 : 4)),
        launch_norm_pix_restore(images, image_dtype, pred, idx_mask, 1, batch, num_mask, e->C, e->img, e->p, pixels, s));
  const int64_t px = (int64_t)batch * e->C * e->img * e->img;
  RUN(TK_DATA, 0, px * (image_dtype == MAE_U8 ? 1 : 4) + pl.Mp * e->P * 4 + px * (out_dtype == MAE_U8 ? 1 : 4) * ((recon != nullptr) + (masked != nullptr)),
      launch_reconstruct_compose(images, image_dtype, pixels, idx_mask, batch, e->C, e->img, e->p, num_mask, fill, out_dtype, recon, masked, stats,
                                 scratch, scratch_bytes, s));
  return 0;
}

extern "C" int mae_engine_backward(mae_engine_t* e, const float* params, const void* wcache, const float* d_pred,
                                   const float* d_x_encoded_extra, int32_t batch, int32_t num_keep, int32_t num_mask,
                                   void* workspace, int64_t workspace_bytes, float* grads, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_backward"));
  MAE_REQUIRE(d_pred && grads, "mae_engine_backward: null d_pred/grads");
  MAE_REQUIRE(num_mask == pl.m && pl.m > 0, "mae_engine_backward: num_mask mismatch");
  Ctx c = make_ctx(e, params, wcache, grads, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_cast(d_pred, MAE_F32, c.buf<>(pl.dpred), e->act, pl.Mp * e->PO, s));
  return backward_impl(c, pl, d_x_encoded_extra);
}

extern "C" int mae_engine_backward_decoder(mae_engine_t* e, const float* params, const void* wcache, const float* d_pred,
                                           int32_t batch, int32_t num_keep, int32_t num_mask, void* workspace,
                                           int64_t workspace_bytes, float* grads, float* d_x_encoded, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_backward_decoder"));
  MAE_REQUIRE(d_pred && grads, "mae_engine_backward_decoder: null d_pred/grads");
  MAE_REQUIRE(num_mask == pl.m && pl.m > 0, "mae_engine_backward_decoder: num_mask mismatch");
  Ctx c = make_ctx(e, params, wcache, grads, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_cast(d_pred, MAE_F32, c.buf<>(pl.dpred), e->act, pl.Mp * e->PO, s));
  backward_begin(c);
  MAE_TRY(backward_decoder_impl(c, pl));
  MAE_TRY(backward_end(c));
  if (d_x_encoded) MAE_TRY(launch_cast(c.buf<>(pl.d_ln), e->act, d_x_encoded, MAE_F32, pl.Me * e->D, s));
  return 0;
}

extern "C" int mae_engine_backward_encoder(mae_engine_t* e, const float* params, const void* wcache, const float* d_x_encoded,
                                           int32_t batch, int32_t num_keep, void* workspace, int64_t workspace_bytes,
                                           float* grads, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, "mae_engine_backward_encoder"));
  MAE_REQUIRE(d_x_encoded && grads, "mae_engine_backward_encoder: null d_x_encoded/grads");
  Ctx c = make_ctx(e, params, wcache, grads, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_cast(d_x_encoded, MAE_F32, c.buf<>(pl.d_ln), e->act, pl.Me * e->D, s));
  backward_begin(c);
  MAE_TRY(backward_encoder_impl(c, pl));
  return backward_end(c);
}

extern "C" int64_t mae_engine_encoder_grad_elems(const mae_engine_t* e) { return e ? e->params[e->i_dec_mask].offset : 0; }

// decoder.decode(x) of lightly MAEDecoderTIMM (src/models/mae.py:71): x + decoder_pos_embed -> blocks -> decoder_norm, every row
extern "C" int mae_engine_decoder_decode(mae_engine_t* e, const float* params, const void* wcache, const float* x, int32_t batch,
                                         void* workspace, int64_t workspace_bytes, float* out, void* stream) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, 1, workspace, workspace_bytes, &pl, "mae_engine_decoder_decode"));
  MAE_REQUIRE(x && out, "mae_engine_decoder_decode: null x/out");
  Ctx c = make_ctx(e, params, wcache, nullptr, workspace, stream);
  hipStream_t s = c.s;
  MAE_TRY(launch_add_rows_pos(x, c.P(e->i_dec_pos), pl.Md, e->L, e->Dd, c.buf<float>(pl.dec_x[0]), s));
  for (int i = 0; i < e->dd; ++i)
    MAE_TRY(block_forward(c, pl, e->dec[i], pl.dec[i], pl.Md, e->Dd, e->Hd, pl.B, e->L, i ? pl.dec[i - 1].x_mid : 0, i > 0, pl.dec_x[i]));
  // the fused add + LayerNorm kernel reads the branch in its OUTPUT dtype: first pass in the activation dtype (forms the last
  // residual sum in dec_x[dd]; its normalised output goes to scratch), second pass writes fp32 rows for the caller
  float* stat = c.buf<float>(pl.dres);  // statistics of all B*L rows (dec_mean / dec_rstd hold the masked rows only)
  MAE_TRY(ln_fwd(c, c.buf<float>(pl.dec[e->dd - 1].x_mid), c.buf<>(pl.branch_b), c.buf<float>(pl.dec_x[e->dd]), nullptr, c.P(e->i_dn_w),
                 c.P(e->i_dn_b), 1e-6f, pl.Md, e->Dd, c.act, c.buf<>(pl.d_ln), stat, stat + pl.Md));
  return ln_fwd(c, c.buf<float>(pl.dec_x[e->dd]), nullptr, nullptr, nullptr, c.P(e->i_dn_w), c.P(e->i_dn_b), 1e-6f, pl.Md, e->Dd, MAE_F32, out,
                stat, stat + pl.Md);
}

static int loss_and_grads_impl(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                               const float* noise, int32_t batch, int32_t num_keep, float grad_scale, void* workspace, int64_t workspace_bytes, float* grads,
                               float* loss_out, int64_t* idx_keep_out, int64_t* idx_mask_out, void* const* ready, void* stream,
                               const char* who) {
  Plan pl;
  MAE_TRY(check_call(e, params, wcache, batch, num_keep, workspace, workspace_bytes, &pl, who));
  MAE_REQUIRE(images && noise && grads && loss_out, "%s: null argument", who);
  MAE_TRY(check_image_dtype(image_dtype, who));
  MAE_REQUIRE(pl.m > 0, "%s: nothing is masked", who);
  Ctx c = make_ctx(e, params, wcache, grads, workspace, stream);
  hipStream_t s = c.s;
  c.ready = ready;
  {
    TimerScope ts(e, TK_DATA, 0, (double)pl.Md * 12, s);
    MAE_TRY(launch_mask_from_noise(noise, batch, e->L, num_keep, idx_keep_out, idx_mask_out, c.buf<int32_t>(pl.keep32), c.buf<int32_t>(pl.mask32), s));
  }
  MAE_TRY(forward_encoder_impl(c, pl, images, image_dtype, nullptr));
  MAE_TRY(forward_decoder_impl(c, pl, nullptr));
  if (e->cfg.norm_pix_loss)
    RUN(TK_LOSS, 0, pl.Mp * e->P * (4 + c.as) + pl.Mp * e->P * (image_dtype == MAE_U8 ? 1 : 4), launch_mse_norm_pix(c.buf<float>(pl.pred), images, image_dtype, c.buf<int32_t>(pl.mask32), 0, batch, pl.m, e->C, e->img, e->p, grad_scale, loss_out, c.buf<>(pl.dpred), e->act, c.buf<float>(pl.loss_scratch), s));
  else  // image bytes counted: the whole uint8 batch (band walk), the masked patches of a float one
    RUN(TK_LOSS, 0, pl.Mp * e->P * (4 + c.as) + (image_dtype == MAE_U8 ? (int64_t)batch * e->C * e->img * e->img : pl.Mp * e->P * 4), launch_mse_from_images(c.buf<float>(pl.pred), images, image_dtype, c.buf<int32_t>(pl.mask32), batch, pl.m, e->C, e->img, e->p, grad_scale, loss_out, c.buf<>(pl.dpred), e->act, c.buf<float>(pl.loss_scratch), 0, s));
  return backward_impl(c, pl);
}

extern "C" int mae_engine_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                                         int32_t image_dtype, const float* noise, int32_t batch, int32_t num_keep, float grad_scale, void* workspace,
                                         int64_t workspace_bytes, float* grads, float* loss_out, int64_t* idx_keep_out,
                                         int64_t* idx_mask_out, void* stream) {
  return loss_and_grads_impl(e, params, wcache, images, image_dtype, noise, batch, num_keep, grad_scale, workspace, workspace_bytes, grads,
                             loss_out, idx_keep_out, idx_mask_out, nullptr, stream, "mae_engine_loss_and_grads");
}

extern "C" int32_t mae_engine_grad_ready_points(const mae_engine_t* e, int64_t* offsets, int32_t max_points) {
  if (!e) return 0;
  const int n = e->depth + 1;
  if (offsets) {
    for (int j = 0; j < n && j < max_points; ++j) {
      if (j == 0) offsets[j] = e->params[e->i_dec_mask].offset;
      else if (j < e->depth) offsets[j] = e->params[e->enc[e->depth - j].ln1_w].offset;
      else offsets[j] = 0;
    }
  }
  return n;
}

extern "C" int mae_engine_loss_and_grads_phased(mae_engine_t* e, const float* params, const void* wcache, const void* images,
                                                int32_t image_dtype, const float* noise, int32_t batch, int32_t num_keep, float grad_scale, void* workspace,
                                                int64_t workspace_bytes, float* grads, float* loss_out, int64_t* idx_keep_out,
                                                int64_t* idx_mask_out, void* const* ready_events, int32_t num_ready, void* stream) {
  MAE_REQUIRE(e, "mae_engine_loss_and_grads_phased: null engine");
  MAE_REQUIRE(ready_events && num_ready == e->depth + 1,
              "mae_engine_loss_and_grads_phased: need one event slot per gradient-ready point (%d), got %d", e->depth + 1, num_ready);
  return loss_and_grads_impl(e, params, wcache, images, image_dtype, noise, batch, num_keep, grad_scale, workspace, workspace_bytes, grads,
                             loss_out, idx_keep_out, idx_mask_out, ready_events, stream, "mae_engine_loss_and_grads_phased");
}

// =====================================================================================================
// I-JEPA step (BASELINE.json configs[2], [4]; NO reference code -- specification: DESIGN.md section "I-JEPA")
//   target encoder (EMA weights, every patch token, no gradient) -> parameter-free LayerNorm -> target rows h
//   context encoder on the context tokens -> predictor on [context | mask tokens of block i] for each target block
//   -> latent regression loss -> backward through predictor and context encoder
// The engine's "decoder" tensors are the predictor (decoder_embed = predictor_embed, decoder_pred: Dd -> D, pred_dim = D).
// =====================================================================================================
namespace mae {

struct JepaPlan {
  int64_t ctx32, tgt32, tgt_rows, ones, zeros, stat, h, phase, total;
  Plan tgt, ctx;   // plans of the two phases, both placed at `phase`
  int64_t xenc;    // fp32 output of the target encoder, behind the target-phase plan
};

static JepaPlan make_jepa_plan(const mae_engine* e, int B, int k, int nblk, int m) {
  JepaPlan jp;
  const int N = e->L - 1;
  int64_t off = 0;
  auto take = [&](int64_t bytes) { const int64_t o = off; off += round_up(std::max<int64_t>(bytes, 4), 256); return o; };
  const int64_t Mp = (int64_t)B * nblk * m;
  jp.ctx32 = take((int64_t)B * k * 4);
  jp.tgt32 = take(Mp * 4);
  jp.tgt_rows = take(Mp * 4);
  jp.ones = take(e->D * 4);
  jp.zeros = take(e->D * 4);
  jp.stat = take(2 * Mp * 4);
  jp.h = take(Mp * e->D * 4);
  jp.phase = off;
  jp.tgt = make_encoder_plan(e, B, false);                       // encoder over every patch token
  jp.xenc = round_up(jp.tgt.total, 256);
  const int64_t tgt_total = jp.xenc + round_up((int64_t)B * N * e->D * 4, 256);
  jp.ctx = make_plan_ex(e, B, k, B * nblk, k + m, m);
  jp.total = jp.phase + std::max(tgt_total, jp.ctx.total);
  return jp;
}

}  // namespace mae

extern "C" int64_t mae_engine_jepa_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_context, int32_t num_blocks,
                                                   int32_t block_tokens) {
  if (!e || batch <= 0 || num_context < 1 || num_context >= e->L || num_blocks < 1 || block_tokens < 1 || block_tokens >= e->L) return -1;
  return make_jepa_plan(e, batch, num_context, num_blocks, block_tokens).total;
}

extern "C" int mae_engine_jepa_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const float* target_params,
                                              const void* target_wcache, const void* images, int32_t image_dtype,
                                              const int64_t* idx_context, const int64_t* idx_target, int32_t batch, int32_t num_context,
                                              int32_t num_blocks, int32_t block_tokens, int32_t loss_kind, float grad_scale,
                                              void* workspace, int64_t workspace_bytes, float* grads, float* loss_out, float* h_out,
                                              float* pred_out, void* const* ready_events, int32_t num_ready, void* stream) {
  const char* who = "mae_engine_jepa_loss_and_grads";
  MAE_TRY(check_common(e, params, wcache, batch, workspace, who));
  MAE_TRY(check_common(e, target_params, target_wcache, batch, workspace, who));  // the EMA arena and its weight cache: same rules
  MAE_REQUIRE(e->PO == e->D, "%s: the engine was not created with pred_dim = embed_dim (I-JEPA predicts latents of the encoder width)", who);
  MAE_REQUIRE(images && idx_context && idx_target && loss_out, "%s: null argument", who);
  MAE_REQUIRE(batch > 0 && num_context >= 1 && num_blocks >= 1 && block_tokens >= 1 && num_context + block_tokens <= e->L - 1 + block_tokens &&
              num_context < e->L && block_tokens < e->L, "%s: bad token counts (context %d, blocks %d x %d, %d patches)", who, num_context, num_blocks, block_tokens, e->L - 1);
  MAE_REQUIRE(loss_kind == MAE_LOSS_MSE || loss_kind == MAE_LOSS_SMOOTH_L1, "%s: loss_kind must be MAE_LOSS_MSE or MAE_LOSS_SMOOTH_L1", who);
  MAE_REQUIRE(!ready_events || num_ready == e->depth + 1, "%s: need one event slot per gradient-ready point (%d)", who, e->depth + 1);
  MAE_TRY(check_image_dtype(image_dtype, who));
  const JepaPlan jp = make_jepa_plan(e, batch, num_context, num_blocks, block_tokens);
  MAE_REQUIRE(workspace_bytes >= jp.total, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, (long long)jp.total);
  hipStream_t s = (hipStream_t)stream;
  char* ws = (char*)workspace;
  const int N = e->L - 1;
  const int64_t Mp = (int64_t)batch * num_blocks * block_tokens;
  int32_t* ctx32 = reinterpret_cast<int32_t*>(ws + jp.ctx32);
  int32_t* tgt32 = reinterpret_cast<int32_t*>(ws + jp.tgt32);
  int32_t* tgt_rows = reinterpret_cast<int32_t*>(ws + jp.tgt_rows);
  float* h = h_out ? h_out : reinterpret_cast<float*>(ws + jp.h);
  MAE_TRY(launch_idx_to_i32(idx_context, ctx32, (int64_t)batch * num_context, s));
  MAE_TRY(launch_idx_to_i32(idx_target, tgt32, Mp, s));
  // ---- phase A: target encoder over all patch tokens (EMA weights), fp32 output, parameter-free LayerNorm of the target rows
  {
    Ctx c = make_ctx(e, target_params, target_wcache, nullptr, ws + jp.phase, stream);
    c.fwd_only = true;
    float* xenc = reinterpret_cast<float*>(ws + jp.phase + jp.xenc);
    MAE_TRY(keep_every_token(c, jp.tgt, false));
    MAE_TRY(forward_encoder_impl(c, jp.tgt, images, image_dtype, xenc));
    MAE_TRY(launch_rows_from_tokens(tgt32, batch, num_blocks * block_tokens, N, tgt_rows, s));
    MAE_TRY(launch_fill(reinterpret_cast<float*>(ws + jp.ones), 1.0f, e->D, s));
    MAE_HIP(hipMemsetAsync(ws + jp.zeros, 0, (size_t)e->D * 4, s));
    float* stat = reinterpret_cast<float*>(ws + jp.stat);
    MAE_TRY(ln_fwd(c, xenc, nullptr, nullptr, tgt_rows, reinterpret_cast<float*>(ws + jp.ones), reinterpret_cast<float*>(ws + jp.zeros),
                   1e-5f, Mp, e->D, MAE_F32, h, stat, stat + Mp));  // F.layer_norm default eps
  }
  if (!grads) return 0;  // targets only
  // ---- phase B: context encoder, predictor, loss, backward
  Ctx c = make_ctx(e, params, wcache, grads, ws + jp.phase, stream);
  c.ready = ready_events;
  const Plan& pl = jp.ctx;
  MAE_HIP(hipMemcpyAsync(c.buf<int32_t>(pl.keep32), ctx32, (size_t)batch * num_context * 4, hipMemcpyDeviceToDevice, s));
  MAE_TRY(forward_encoder_impl(c, pl, images, image_dtype, nullptr));
  const JepaSeq seq{ctx32, tgt32, num_blocks};
  MAE_TRY(forward_decoder_impl(c, pl, pred_out, &seq));
  const float* pred = pred_out ? pred_out : c.buf<float>(pl.pred);
  if (loss_kind == MAE_LOSS_SMOOTH_L1)
    RUN(TK_LOSS, 0, Mp * e->D * (8 + c.as), launch_smooth_l1(pred, h, Mp * e->D, grad_scale, loss_out, c.buf<>(pl.dpred), e->act, c.buf<float>(pl.loss_scratch), s));
  else
    RUN(TK_LOSS, 0, Mp * e->D * (8 + c.as), launch_mse(pred, h, Mp * e->D, grad_scale, loss_out, c.buf<>(pl.dpred), e->act, c.buf<float>(pl.loss_scratch), s));
  return backward_impl(c, pl, nullptr, &seq);
}

// Adam's bias corrections 1 - beta^step of the 1-based step, computed in double
struct AdamBias { float c1, c2; };
static AdamBias adam_bias(float beta1, float beta2, int64_t step) {
  return {(float)(1.0 - std::pow((double)beta1, (double)step)), (float)(1.0 - std::pow((double)beta2, (double)step))};
}

// [lo, lo + count) lies inside the trainable range of the arena, on 4-element boundaries (the optimizer kernels take multiples of 4 elements)
static int check_arena_range(const mae_engine* e, int64_t lo, int64_t count, const char* who) {
  MAE_REQUIRE(lo >= 0 && count >= 0 && lo % 4 == 0 && count % 4 == 0 && lo + count <= e->trainable_elems,
              "%s: range [%lld, +%lld) outside the %lld trainable elements or not a multiple of 4", who, (long long)lo, (long long)count,
              (long long)e->trainable_elems);
  return 0;
}

static int optimizer_step_impl(mae_engine_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* wcache,
                               float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, int64_t step,
                               float* stats_out, float* scratch, float* ema_target, void* ema_wcache, float ema_momentum, void* stream) {
  MAE_REQUIRE(e && params && grads && exp_avg && exp_avg_sq && stats_out && scratch, "mae_engine_optimizer_step: null argument");
  MAE_REQUIRE(step >= 1, "mae_engine_optimizer_step: step is 1-based");
  MAE_REQUIRE(e->act == MAE_F32 || wcache, "mae_engine_optimizer_step: bf16 engine needs the weight cache");
  hipStream_t s = (hipStream_t)stream;
  const int64_t n = e->trainable_elems;
  const AdamBias bc = adam_bias(beta1, beta2, step);
  RUN(TK_OPTIM, 0, n * 4, launch_grad_norm(grads, n, max_norm, stats_out, scratch, s));
  RUN(TK_OPTIM, 0, n * (28 + (e->act == MAE_BF16 ? 2 : 0)),
      launch_adamw(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, bc.c1, bc.c2, stats_out,
                   e->act == MAE_BF16 ? reinterpret_cast<bf16*>(wcache) : nullptr, s, ema_target,
                   e->act == MAE_BF16 ? reinterpret_cast<bf16*>(ema_wcache) : nullptr, ema_target ? e->params[e->i_dec_mask].offset : 0, ema_momentum));
  if (e->act == MAE_BF16) RUN(TK_OPTIM, 0, e->trans_elems * 6, refresh_transposed(e, params, wcache, s));
  return 0;
}

extern "C" int mae_engine_optimizer_step(mae_engine_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* wcache,
                                         float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, int64_t step,
                                         float* stats_out, float* scratch, void* stream) {
  return optimizer_step_impl(e, params, grads, exp_avg, exp_avg_sq, wcache, lr, beta1, beta2, eps, weight_decay, max_norm, step, stats_out,
                             scratch, nullptr, nullptr, 0.f, stream);
}

// ---- optimizer on a shard of the arena (data-parallel ranks that own 1 / world of the parameters) ----------------
extern "C" int mae_engine_grad_sumsq_range(mae_engine_t* e, const float* grads, int64_t lo, int64_t count, float* sumsq_out, float* scratch,
                                           void* stream) {
  MAE_REQUIRE(e && grads && sumsq_out && scratch, "mae_engine_grad_sumsq_range: null argument");
  MAE_TRY(check_arena_range(e, lo, count, "mae_engine_grad_sumsq_range"));
  return launch_grad_sumsq(grads + lo, count, sumsq_out, scratch, (hipStream_t)stream);
}

extern "C" int mae_engine_clip_from_sumsq(mae_engine_t* e, const float* sumsq, float max_norm, float* stats_out, void* stream) {
  MAE_REQUIRE(e && sumsq && stats_out, "mae_engine_clip_from_sumsq: null argument");
  return launch_clip_from_sumsq(sumsq, max_norm, stats_out, (hipStream_t)stream);
}

extern "C" int mae_engine_adamw_range(mae_engine_t* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, void* wcache,
                                      float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* stats,
                                      int64_t lo, int64_t count, void* stream) {
  MAE_REQUIRE(e && params && grads && exp_avg && exp_avg_sq && stats, "mae_engine_adamw_range: null argument");
  MAE_REQUIRE(step >= 1, "mae_engine_adamw_range: step is 1-based");
  MAE_TRY(check_arena_range(e, lo, count, "mae_engine_adamw_range"));
  MAE_REQUIRE(e->act == MAE_F32 || wcache, "mae_engine_adamw_range: bf16 engine needs the weight cache");
  if (count == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const AdamBias bc = adam_bias(beta1, beta2, step);
  RUN(TK_OPTIM, 0, count * (28 + (e->act == MAE_BF16 ? 2 : 0)),
      launch_adamw(params + lo, grads + lo, exp_avg + lo, exp_avg_sq + lo, count, lr, beta1, beta2, eps, weight_decay, bc.c1, bc.c2, stats,
                   e->act == MAE_BF16 ? reinterpret_cast<bf16*>(wcache) + lo : nullptr, s));
  return 0;   // the bf16 operand copies of the OTHER ranks' shards and the transposes: mae_engine_refresh_weights after the all-gather
}

// ---- gradient accumulation over micro-batches (DESIGN section "Gradient accumulation") ---------------------------------------
// The buffers are the caller's (a gradient arena with its tail, a head or position gradient): no range of the engine bounds them.
extern "C" int mae_engine_grad_accumulate(mae_engine_t* e, float* dst, const float* src, int64_t lo, int64_t count, int32_t overwrite,
                                          void* stream) {
  MAE_REQUIRE(e && dst && src, "mae_engine_grad_accumulate: null argument");
  MAE_REQUIRE(lo >= 0 && count >= 0 && lo % 4 == 0 && count % 4 == 0, "mae_engine_grad_accumulate: range [%lld, +%lld) is not a multiple of 4",
              (long long)lo, (long long)count);
  MAE_REQUIRE(((uintptr_t)(dst + lo) | (uintptr_t)(src + lo)) % 16 == 0, "mae_engine_grad_accumulate: dst + lo and src + lo must be 16-byte aligned");
  if (count == 0) return 0;
  MAE_REQUIRE((uintptr_t)(dst + lo + count) <= (uintptr_t)(src + lo) || (uintptr_t)(src + lo + count) <= (uintptr_t)(dst + lo),
              "mae_engine_grad_accumulate: dst and src overlap");
  hipStream_t s = (hipStream_t)stream;
  RUN(TK_OPTIM, 0, count * (overwrite ? 8 : 12), launch_grad_accumulate(dst + lo, src + lo, count, overwrite != 0, s));
  return 0;
}

extern "C" int mae_engine_optimizer_step_ema(mae_engine_t* e, float* params, float* grads, float* exp_avg, float* exp_avg_sq, void* wcache,
                                             float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm, int64_t step,
                                             float* stats_out, float* scratch, float* target_params, void* target_wcache,
                                             float ema_momentum, void* stream) {
  MAE_REQUIRE(target_params && (!e || e->act == MAE_F32 || target_wcache), "mae_engine_optimizer_step_ema: null target arena / weight cache");
  MAE_REQUIRE(ema_momentum >= 0.f && ema_momentum <= 1.f, "mae_engine_optimizer_step_ema: momentum %g outside [0, 1]", (double)ema_momentum);
  return optimizer_step_impl(e, params, grads, exp_avg, exp_avg_sq, wcache, lr, beta1, beta2, eps, weight_decay, max_norm, step, stats_out,
                             scratch, target_params, target_wcache, ema_momentum, stream);
}

// =====================================================================================================
// Downstream classifier (src/models/classifier.py:47-57, src/training/classifier.py:75-171): the encoder over every token,
// the pooled head + cross-entropy (k_classifier.hip) and a backward that stops where the trainable suffix ends.
//   train_blocks = -1: linear probe -- the forward saves nothing for a backward, only the head gets gradients;
//   train_blocks = n : final LayerNorm + blocks[depth-n:] (unfreeze_last_layers(n)); nothing below them runs;
//   train_embed  = 1 : (n = depth only) also cls_token, the patch projection and pos_embed (unfreeze_encoder()).
// Every entry point is one ClsCall handed to classifier_impl: the wider ones (_ex: the patch-only sequence, with_cls = 0, tokens
// 1..N, what an I-JEPA encoder was trained on, and the patch-row mean MAE_POOL_MEAN_PATCHES; _soft: soft targets; _sd: drop path)
// set more of its fields, and a field left at its default issues the narrower entry's launches.
// =====================================================================================================
namespace mae {

struct ClsPlan {
  Plan pl;  // the full-sequence plan (num_keep = L, or L - 1 without the class token) at offset 0; the classifier's own buffers follow it
  int64_t pooled, dlogits, row_loss, row_correct, dpooled, mean_c, rstd_c, cls_rows, head_partial, head_sum, pos_partial, total;
};

static ClsPlan make_cls_plan(const mae_engine* e, int B, int C, bool with_cls = true) {
  ClsPlan cp;
  cp.pl = with_cls ? make_plan(e, B, e->L) : make_encoder_plan(e, B, false);
  const int T = cp.pl.k;
  int64_t off = round_up(cp.pl.total, 256);
  auto take = [&](int64_t bytes) { const int64_t o = off; off += round_up(std::max<int64_t>(bytes, 4), 256); return o; };
  const int64_t D = e->D;
  cp.pooled = take(B * D * 4);
  cp.dlogits = take((int64_t)B * C * 4);
  cp.row_loss = take((int64_t)B * 4);
  cp.row_correct = take((int64_t)B * 4);
  cp.dpooled = take(B * D * 4);
  cp.mean_c = take((int64_t)B * 4);
  cp.rstd_c = take((int64_t)B * 4);
  cp.cls_rows = take((int64_t)B * 4);
  cp.head_partial = take(classifier_wgrad_partial_floats(B, C, e->D) * 4);
  cp.head_sum = take(round_up((int64_t)C * D + C, 4) * 4);
  cp.pos_partial = take((int64_t)full_grad_split_slices(B, T, e->D) * T * D * 4);
  cp.total = off;
  return cp;
}

// One classifier call: what the six entry points take, the defaults being the first entry's (forward over [cls | patches]).
struct ClsCall {
  const float *params = nullptr, *head = nullptr;
  const void *wcache = nullptr, *images = nullptr;
  const int64_t* labels = nullptr;
  int32_t image_dtype = MAE_F32, batch = 0, with_cls = 1, pool = MAE_POOL_CLS, num_classes = 0, train_blocks = -1, train_embed = 0;
  bool extended_pools = false;  // the entry takes with_cls = 0 and MAE_POOL_MEAN_PATCHES
  bool training = false;        // a loss_and_grads entry: head_grads is required
  float grad_scale = 1.f;
  void *workspace = nullptr, *stream = nullptr;
  int64_t workspace_bytes = 0;
  float *grads = nullptr, *head_grads = nullptr, *pos_grad = nullptr, *logits = nullptr, *loss_out = nullptr;
  int32_t* correct_out = nullptr;
  HeadSoft soft = {nullptr, nullptr, 0.f};  // inactive: the hard-label kernels
  const float* branch_scale = nullptr;      // drop path; null: none
};
// The six entry points name their parameters alike, so each fills its record from them with these: what every entry takes, and what
// the four loss_and_grads entries add.
#define CLS_CALL(k)                                                                                                                    \
  ClsCall k;                                                                                                                           \
  k.params = params; k.wcache = wcache; k.head = head; k.images = images; k.image_dtype = image_dtype; k.labels = labels;              \
  k.batch = batch; k.pool = pool; k.num_classes = num_classes; k.workspace = workspace; k.workspace_bytes = workspace_bytes;           \
  k.logits = logits; k.loss_out = loss_out; k.correct_out = correct_out; k.stream = stream
#define CLS_CALL_TRAINING(k)                                                                                                           \
  k.training = true; k.train_blocks = train_blocks; k.train_embed = train_embed; k.grad_scale = grad_scale;                            \
  k.grads = grads; k.head_grads = head_grads; k.pos_grad = pos_grad

static int classifier_impl(mae_engine* e, const ClsCall& k, const char* who) {
  if (k.training) MAE_REQUIRE(k.head_grads, "%s: null head_grads", who);
  else MAE_REQUIRE(k.labels || (!k.loss_out && !k.correct_out), "%s: loss / correct count need labels", who);
  MAE_REQUIRE(k.soft.eps >= 0.f && k.soft.eps < 1.f, "%s: label_smoothing = %g outside [0, 1)", who, (double)k.soft.eps);
  MAE_TRY(check_common(e, k.params, k.wcache, k.batch, k.workspace, who));
  const int32_t train_blocks = k.train_blocks;
  MAE_REQUIRE(!k.branch_scale || (k.head_grads && train_blocks >= 0),
              "%s: branch_scale needs a training encoder (train_blocks >= 0); the probe's encoder is in inference and never drops", who);
  MAE_REQUIRE(k.batch > 0, "%s: batch %d out of range", who, k.batch);
  MAE_REQUIRE(k.head && k.images, "%s: null head/images", who);
  MAE_TRY(check_image_dtype(k.image_dtype, who));
  MAE_REQUIRE(k.num_classes >= 2 && k.num_classes <= HEAD_MAX_CLASSES, "%s: num_classes = %d outside [2, %d]", who, k.num_classes, HEAD_MAX_CLASSES);
  MAE_TRY(check_pool(k.with_cls, k.pool, k.extended_pools, who));
  if (k.extended_pools) MAE_REQUIRE(e->L >= 2 && e->D % 4 == 0 && e->D <= 1024, "%s: needs a patch row and embed_dim a multiple of 4 up to 1024", who);
  const bool with_cls = k.with_cls != 0;
  const ClsPlan cp = make_cls_plan(e, k.batch, k.num_classes, with_cls);
  const Plan& pl = cp.pl;
  MAE_REQUIRE(k.workspace_bytes >= cp.total, "%s: workspace too small (%lld < %lld bytes)", who, (long long)k.workspace_bytes, (long long)cp.total);
  const bool train = k.head_grads != nullptr;
  if (train) {
    MAE_REQUIRE(k.labels && k.loss_out, "%s: training needs labels and loss_out", who);
    MAE_REQUIRE(train_blocks >= -1 && train_blocks <= e->depth, "%s: train_blocks = %d outside [-1, %d]", who, train_blocks, e->depth);
    MAE_REQUIRE(k.train_embed == 0 || (k.train_embed == 1 && train_blocks == e->depth),
                "%s: train_embed = 1 needs train_blocks = depth (%d), got %d", who, e->depth, train_blocks);
    MAE_REQUIRE(train_blocks < 0 || k.grads, "%s: train_blocks >= 0 needs the gradient arena", who);
    MAE_REQUIRE(!k.train_embed || k.pos_grad, "%s: train_embed needs the pos_embed gradient buffer", who);
  }
  Ctx c = make_ctx(e, k.params, k.wcache, k.grads, k.workspace, k.stream);
  hipStream_t s = c.s;
  const bool enc_bwd = train && train_blocks >= 0;
  c.fwd_only = !enc_bwd;  // the linear probe and evaluation save no GELU derivative
  c.branch_scale = k.branch_scale;
  const int B = k.batch, L = pl.k, D = e->D, C = k.num_classes;  // L rows per image: the class token (if any) and every patch
  MAE_TRY(keep_every_token(c, pl, with_cls));
  MAE_TRY(forward_encoder_impl(c, pl, k.images, k.image_dtype, nullptr));
  const bool cls = k.pool == MAE_POOL_CLS;
  HeadCall h;
  h.feats = c.buf<>(pl.enc_norm); h.dt = e->act; h.B = B; h.seq = L; h.D = D; h.with_cls = k.with_cls; h.pool = k.pool;
  h.W = k.head; h.bias = k.head + (int64_t)C * D; h.C = C; h.labels = k.labels; h.soft = k.soft; h.grad_scale = k.grad_scale;
  h.logits_out = k.logits; h.row_loss = c.buf<float>(cp.row_loss); h.row_correct = c.buf<int32_t>(cp.row_correct);
  h.loss_out = k.loss_out; h.correct_out = k.correct_out;
  h.pooled_out = train ? c.buf<float>(cp.pooled) : nullptr; h.dlogits_out = train ? c.buf<float>(cp.dlogits) : nullptr;
  h.dfeat_out = enc_bwd ? (cls ? c.buf<>(cp.dpooled) : c.buf<>(pl.d_ln)) : nullptr;
  h.mean_all = c.buf<float>(pl.enc_mean); h.rstd_all = c.buf<float>(pl.enc_rstd); h.mean_c = c.buf<float>(cp.mean_c); h.rstd_c = c.buf<float>(cp.rstd_c);
  h.cls_rows = enc_bwd && cls ? c.buf<int32_t>(cp.cls_rows) : nullptr;
  // bytes: the rows the head reads (the patch rows, the class row or every row), W, and the (B * L, D) feature gradient of a mean pool
  const double rows_read = h.range() ? (double)B * (L - k.with_cls) : cls ? (double)B : (double)pl.Me;
  RUN(TK_LOSS, 2.0 * B * C * D * (train ? 2 : 1), rows_read * D * c.as + (double)C * D * 4 + (enc_bwd && !cls ? (double)pl.Me * D * c.as : 0.0),
      launch_classifier_head(h, s));
  if (!train) return 0;
  RUN(TK_WGRAD, 2.0 * B * C * D, (double)B * (C + D) * 4, launch_classifier_head_wgrad(c.buf<float>(cp.dlogits), c.buf<float>(cp.pooled), B, C, D,
                                                                                    c.buf<float>(cp.head_partial), c.buf<float>(cp.head_sum), k.head_grads, s));
  if (!enc_bwd) return 0;
  float* dres = c.buf<float>(pl.dres);
  backward_begin(c);
  if (cls) {
    // only the B class-token rows carry gradient: zero the rest of the residual gradient, then a row-mapped final LayerNorm backward
    RUN(TK_DATA, 0, (pl.Me - B) * D * (4 + c.as), launch_zero_token_rows(pl.Me, L, D, e->act, dres, c.buf<>(pl.dres_c), s));
    MAE_TRY(ln_bwd(c, pl, c.buf<>(cp.dpooled), c.buf<float>(pl.enc_x[e->depth]), c.buf<int32_t>(cp.cls_rows), e->i_norm_w, e->i_norm_b,
                   c.buf<float>(cp.mean_c), c.buf<float>(cp.rstd_c), B, D, 0, c.scale_row(2 * e->depth - 1, B), L));
  } else {
    MAE_TRY(ln_bwd(c, pl, c.buf<>(pl.d_ln), c.buf<float>(pl.enc_x[e->depth]), nullptr, e->i_norm_w, e->i_norm_b, c.buf<float>(pl.enc_mean),
                   c.buf<float>(pl.enc_rstd), pl.Me, D, 0, c.scale_row(2 * e->depth - 1, B), L));
  }
  for (int i = e->depth - 1; i >= e->depth - train_blocks; --i)  // the trainable suffix only: the sweep stops below blocks[depth-n]
    MAE_TRY(block_backward(c, pl, e->enc[i], pl.enc[i], pl.Me, D, e->H, B, L, pl.enc_x[i], i ? c.scale_row(2 * i - 1, B) : nullptr,
                           c.scale_row(2 * i, B)));
  if (k.train_embed) {
    // token assembly: d pos_embed, d cls_token and the patch rows from one read of dres, then the patch projection.  Without a class
    // row every row feeds the patch projection; pos_embed[0] and cls_token get exact zeros
    RUN(TK_DATA, 0, pl.Me * D * (4 + c.as), launch_full_grad_split(dres, B, L, D, e->act, c.buf<>(pl.dtok), k.pos_grad, c.Gp(e->i_cls),
                                                                  c.buf<float>(cp.pos_partial), with_cls, s));
    MAE_TRY(wgrad(c, pl, c.buf<>(pl.dtok), c.buf<>(pl.patchA), pl.Me, D, e->P, e->i_patch_w, e->i_patch_b));
  }
  return backward_end(c);
}

}  // namespace mae

extern "C" int64_t mae_engine_classifier_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t num_classes) {
  if (!e || batch <= 0 || num_classes < 2 || num_classes > HEAD_MAX_CLASSES) return -1;
  return make_cls_plan(e, batch, num_classes).total;
}

extern "C" int mae_engine_classifier_forward(mae_engine_t* e, const float* params, const void* wcache, const float* head, const void* images,
                                             int32_t image_dtype, const int64_t* labels, int32_t batch, int32_t pool, int32_t num_classes,
                                             void* workspace, int64_t workspace_bytes, float* logits, float* loss_out, int32_t* correct_out,
                                             void* stream) {
  CLS_CALL(k);
  return classifier_impl(e, k, "mae_engine_classifier_forward");
}

extern "C" int mae_engine_classifier_loss_and_grads(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                                    const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                                    int32_t pool, int32_t num_classes, int32_t train_blocks, int32_t train_embed,
                                                    float grad_scale, void* workspace, int64_t workspace_bytes, float* grads,
                                                    float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                                    int32_t* correct_out, void* stream) {
  CLS_CALL(k);
  CLS_CALL_TRAINING(k);
  return classifier_impl(e, k, "mae_engine_classifier_loss_and_grads");
}

extern "C" int64_t mae_engine_classifier_workspace_bytes_ex(const mae_engine_t* e, int32_t batch, int32_t num_classes, int32_t with_cls) {
  if (!e || batch <= 0 || num_classes < 2 || num_classes > HEAD_MAX_CLASSES || (with_cls != 0 && with_cls != 1) || e->L < 2) return -1;
  if (!batch_in_bound(e, batch)) return -1;
  return make_cls_plan(e, batch, num_classes, with_cls != 0).total;
}

extern "C" int mae_engine_classifier_forward_ex(mae_engine_t* e, const float* params, const void* wcache, const float* head, const void* images,
                                                int32_t image_dtype, const int64_t* labels, int32_t batch, int32_t with_cls, int32_t pool,
                                                int32_t num_classes, void* workspace, int64_t workspace_bytes, float* logits, float* loss_out,
                                                int32_t* correct_out, void* stream) {
  CLS_CALL(k);
  k.with_cls = with_cls; k.extended_pools = true;
  return classifier_impl(e, k, "mae_engine_classifier_forward_ex");
}

extern "C" int mae_engine_classifier_loss_and_grads_ex(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                                       const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                                       int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                                       int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                                       float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                                       int32_t* correct_out, void* stream) {
  CLS_CALL(k);
  CLS_CALL_TRAINING(k);
  k.with_cls = with_cls; k.extended_pools = true;
  return classifier_impl(e, k, "mae_engine_classifier_loss_and_grads_ex");
}

// mae_engine_classifier_loss_and_grads_ex with the head's soft targets; with nothing soft asked for, the same launches and bits
extern "C" int mae_engine_classifier_loss_and_grads_soft(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                                         const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                                         int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                                         int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                                         float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                                         int32_t* correct_out, const int64_t* labels_b, const float* lam,
                                                         float label_smoothing, void* stream) {
  CLS_CALL(k);
  CLS_CALL_TRAINING(k);
  k.with_cls = with_cls; k.extended_pools = true;
  k.soft = {labels_b, lam, label_smoothing};
  return classifier_impl(e, k, "mae_engine_classifier_loss_and_grads_soft");
}

// mae_engine_classifier_loss_and_grads_soft with stochastic depth: branch_scale (2 * depth, batch) scales each image's residual branches
extern "C" int mae_engine_classifier_loss_and_grads_sd(mae_engine_t* e, const float* params, const void* wcache, const float* head,
                                                       const void* images, int32_t image_dtype, const int64_t* labels, int32_t batch,
                                                       int32_t with_cls, int32_t pool, int32_t num_classes, int32_t train_blocks,
                                                       int32_t train_embed, float grad_scale, void* workspace, int64_t workspace_bytes,
                                                       float* grads, float* head_grads, float* pos_grad, float* logits, float* loss_out,
                                                       int32_t* correct_out, const int64_t* labels_b, const float* lam,
                                                       float label_smoothing, const float* branch_scale, void* stream) {
  CLS_CALL(k);
  CLS_CALL_TRAINING(k);
  k.with_cls = with_cls; k.extended_pools = true;
  k.soft = {labels_b, lam, label_smoothing};
  k.branch_scale = branch_scale;
  return classifier_impl(e, k, "mae_engine_classifier_loss_and_grads_sd");
}

#undef CLS_CALL
#undef CLS_CALL_TRAINING

// =====================================================================================================
// Frozen-encoder features (scripts/evaluation/visualize_representation.py:87-108): the encoder over [cls | patches] or the
// patches alone, forward only, with a token-sized decoder stub (the I-JEPA target phase's plan).  The encoder stops before
// its final LayerNorm; k_representation.hip does that add + LayerNorm (fp32) + pool + L2 after each block asked for and writes only
// (batch, blocks, W).  The attention maps and the token rows below are read-outs of the same forward.
// =====================================================================================================
extern "C" int64_t mae_engine_features_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls) {
  if (!e || batch <= 0 || (with_cls != 0 && with_cls != 1) || e->D % 4 != 0 || e->D > 1024) return -1;  // the feature kernel's width limit
  if (!batch_in_bound(e, batch)) return -1;
  return make_encoder_plan(e, batch, with_cls != 0).total;
}

// What the four frozen read-outs share, all of it before any launch: the common rules, the images, the plan over every token of every
// image with its workspace size, and a forward-only Ctx.  The entry adds its own rules, then calls run_frozen_forward.
static int begin_frozen_forward(mae_engine* e, const float* params, const void* wcache, const void* images, int image_dtype, int batch,
                                int with_cls, void* workspace, int64_t workspace_bytes, void* stream, const char* who, Plan* pl, Ctx* c) {
  MAE_TRY(check_common(e, params, wcache, batch, workspace, who));
  MAE_REQUIRE(images, "%s: null argument", who);
  MAE_REQUIRE(with_cls == 0 || with_cls == 1, "%s: with_cls must be 0 or 1 (got %d)", who, with_cls);
  MAE_TRY(check_image_dtype(image_dtype, who));
  MAE_REQUIRE(batch > 0, "%s: batch %d out of range", who, batch);
  *pl = make_encoder_plan(e, batch, with_cls != 0);
  MAE_REQUIRE(workspace_bytes >= pl->total, "%s: workspace too small (%lld < %lld bytes)", who, (long long)workspace_bytes, (long long)pl->total);
  *c = make_ctx(e, params, wcache, nullptr, workspace, stream);
  c->fwd_only = true;
  return 0;
}

// The encoder over every token, through block c.last_block: x_mid + branch_b of that block is what the entry reads next.
static int run_frozen_forward(const Ctx& c, const Plan& pl, const void* images, int image_dtype, int with_cls) {
  MAE_TRY(keep_every_token(c, pl, with_cls != 0));
  return forward_encoder_impl(c, pl, images, image_dtype, nullptr);
}

static int check_layers(const mae_engine* e, const int32_t* layers, int n, const char* who) {
  MAE_REQUIRE(n >= 1 && n <= e->depth, "%s: num_layers = %d outside [1, depth = %d]", who, n, e->depth);
  for (int i = 0; i < n; ++i) {
    MAE_REQUIRE(layers[i] >= 0 && layers[i] < e->depth, "%s: layers[%d] = %d outside [0, depth = %d)", who, i, layers[i], e->depth);
    MAE_REQUIRE(i == 0 || layers[i] > layers[i - 1], "%s: layers must be strictly ascending (layers[%d] = %d after %d)", who, i, layers[i], layers[i - 1]);
  }
  return 0;
}

// Both feature calls: the forward with a tap list, stopped after the highest tapped block.  The plain call (`plain`, no list) taps the
// last block alone, keeps to the three single pools and takes any 4-byte aligned feats; the 16-byte rule is the layer call's alone.
static int extract_features_impl(mae_engine* e, const float* params, const void* wcache, const void* images, int image_dtype, int batch,
                                 int with_cls, int pool, int normalize, bool plain, const int32_t* layers, int num_layers, void* workspace,
                                 int64_t workspace_bytes, float* feats, void* stream, const char* who) {
  Plan pl;
  Ctx c{};
  MAE_TRY(begin_frozen_forward(e, params, wcache, images, image_dtype, batch, with_cls, workspace, workspace_bytes, stream, who, &pl, &c));
  MAE_REQUIRE(feats && (plain || layers), "%s: null argument", who);
  if (!plain && pool == MAE_POOL_CLS_MEAN_PATCHES)
    MAE_REQUIRE(with_cls == 1, "%s: pool MAE_POOL_CLS_MEAN_PATCHES needs with_cls = 1 (got %d)", who, with_cls);
  else
    MAE_TRY(check_pool(with_cls, pool, true, who));
  MAE_REQUIRE(e->D % 4 == 0 && e->D <= 1024, "%s: embed_dim = %d must be a multiple of 4 and at most 1024", who, e->D);
  MAE_REQUIRE(normalize == MAE_FEAT_NONE || normalize == MAE_FEAT_L2, "%s: normalize must be MAE_FEAT_NONE or MAE_FEAT_L2 (got %d)", who, normalize);
  const int32_t last = e->depth - 1;
  if (plain) {
    layers = &last;
    num_layers = 1;
  } else {
    MAE_TRY(check_layers(e, layers, num_layers, who));
    MAE_REQUIRE(((uintptr_t)feats & 15) == 0, "%s: feats must be 16-byte aligned", who);
  }
  MAE_REQUIRE(pool == MAE_POOL_CLS || pool == MAE_POOL_MEAN || pl.k > with_cls, "%s: the sequence of %d rows has no patch row", who, pl.k);
  c.tap_layers = layers; c.tap_n = num_layers; c.tap_with_cls = with_cls; c.tap_pool = pool; c.tap_normalize = normalize; c.tap_out = feats;
  c.last_block = layers[num_layers - 1];
  return run_frozen_forward(c, pl, images, image_dtype, with_cls);
}

extern "C" int mae_engine_extract_features(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                           int32_t batch, int32_t with_cls, int32_t pool, int32_t normalize, void* workspace,
                                           int64_t workspace_bytes, float* feats, void* stream) {
  return extract_features_impl(e, params, wcache, images, image_dtype, batch, with_cls, pool, normalize, true, nullptr, 0, workspace, workspace_bytes,
                               feats, stream, "mae_engine_extract_features");
}

// mae_engine_extract_features after the blocks `layers` names, with the fourth pool [class row | patch mean]
extern "C" int mae_engine_extract_layer_features(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                                 int32_t batch, int32_t with_cls, int32_t pool, int32_t normalize, const int32_t* layers,
                                                 int32_t num_layers, void* workspace, int64_t workspace_bytes, float* feats, void* stream) {
  return extract_features_impl(e, params, wcache, images, image_dtype, batch, with_cls, pool, normalize, false, layers, num_layers, workspace,
                               workspace_bytes, feats, stream, "mae_engine_extract_layer_features");
}

// =====================================================================================================
// Attention maps.  A forward-only pass keeps every block's qkv in the workspace (pl.enc[i].qkv), so after a forward
// that stops at the highest block named the maps are column sums of the attention probabilities (k_attnmap.hip) over those buffers:
// the query's start weight w (the class row, or 1 / T) gives maps[:, i] from block layers[i], and the rollout row is the chain
// r <- r / 2 + mean_h S_h(r) / 2 from the top block down to block 0.  Two (batch, T) weight rows ping-pong in pl.dres, which only a
// backward pass uses; the last step writes the caller's buffer.
// =====================================================================================================
extern "C" int64_t mae_engine_attention_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls) {
  return mae_engine_features_workspace_bytes(e, batch, with_cls);
}

// One colsum launch over block l.  `dense` says whether every row of w may be non-zero (the kernel skips the zero rows of a one-hot
// start weight).  Flops: the scores and the weighted sum of the rows that run; bytes: K once, those rows of q, w, the outputs.
static int attention_colsum(const Ctx& c, const Plan& pl, int l, const float* w, bool dense, float* per_head, int64_t stride, float* mixed) {
  mae_engine* e = c.e; hipStream_t s = c.s;
  const int T = pl.k, hd = e->D / e->H;
  const double rows = dense ? T : 1, BH = (double)pl.B * e->H;
  RUN(TK_ATTN_FWD, BH * rows * T * (2.0 * hd + 6), BH * (T + rows) * hd * c.as + (double)pl.B * T * 4 * (1 + (mixed ? 1 : 0) + (per_head ? e->H : 0)),
      launch_attention_colsum(c.buf<>(pl.enc[l].qkv), e->act, pl.B, T, e->H, hd, w, per_head, stride, mixed, s));
  return 0;
}

extern "C" int mae_engine_extract_attention(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                            int32_t batch, int32_t with_cls, int32_t query, const int32_t* layers, int32_t num_layers,
                                            float* maps, float* rollout, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* who = "mae_engine_extract_attention";
  Plan pl;
  Ctx c{};
  MAE_TRY(begin_frozen_forward(e, params, wcache, images, image_dtype, batch, with_cls, workspace, workspace_bytes, stream, who, &pl, &c));
  MAE_REQUIRE(layers && (maps || rollout), "%s: null argument (images, layers, or both of maps and rollout)", who);
  MAE_REQUIRE(query == MAE_ATTN_QUERY_CLS || query == MAE_ATTN_QUERY_MEAN, "%s: query must be MAE_ATTN_QUERY_CLS or MAE_ATTN_QUERY_MEAN (got %d)", who, query);
  MAE_REQUIRE(query != MAE_ATTN_QUERY_CLS || with_cls == 1, "%s: query MAE_ATTN_QUERY_CLS needs with_cls = 1", who);
  MAE_TRY(check_layers(e, layers, num_layers, who));
  MAE_REQUIRE(((uintptr_t)maps & 15) == 0 && ((uintptr_t)rollout & 15) == 0, "%s: maps and rollout must be 16-byte aligned", who);
  const int T = pl.k, H = e->H, hd = e->D / H;
  // the colsum launcher's own limits, so that no forward runs for a call it would refuse
  const int max_t = attention_colsum_max_tokens(hd, e->act);
  MAE_REQUIRE(max_t > 0 && H <= 16, "%s: head_dim %d (16, 24, 32, 48, 64) / %d heads (at most 16) unsupported", who, hd, H);
  MAE_REQUIRE(T >= 1 && T <= max_t, "%s: the sequence of %d tokens is outside the map kernel's [1, %d] at head_dim %d", who, T, max_t, hd);
  MAE_REQUIRE(pl.Me < (1ll << 31), "%s: batch * T = %lld must stay below 2^31", who, (long long)pl.Me);
  const int top = c.last_block = layers[num_layers - 1];
  MAE_TRY(run_frozen_forward(c, pl, images, image_dtype, with_cls));
  float* r[2] = {c.buf<float>(pl.dres), c.buf<float>(pl.dres) + round_up(pl.Me, 4)};   // plan buffers are at least 256 bytes: both fit
  hipStream_t s = c.s;
  RUN(TK_DATA, 0, pl.Me * 4, launch_attention_weight_fill(r[0], batch, T, query == MAE_ATTN_QUERY_CLS ? 0 : -1, s));
  const bool dense0 = query != MAE_ATTN_QUERY_CLS;
  const int64_t stride = (int64_t)num_layers * H * T;
  // the last map is block `top`, the chain's first step: that launch writes both
  float* first = !rollout ? nullptr : top == 0 ? rollout : r[1];
  for (int i = 0; i < num_layers; ++i) {
    float* ph = maps ? maps + (int64_t)i * H * T : nullptr;
    float* mx = i == num_layers - 1 ? first : nullptr;
    if (ph || mx) MAE_TRY(attention_colsum(c, pl, layers[i], r[0], dense0, ph, stride, mx));
  }
  for (int l = top - 1, cur = 1; rollout && l >= 0; --l, cur ^= 1)
    MAE_TRY(attention_colsum(c, pl, l, r[cur], true, nullptr, 0, l == 0 ? rollout : r[cur ^ 1]));
  return 0;
}

// mae_engine_extract_features without the pool: the same encoder forward, then the last residual add and the final LayerNorm in fp32
// (launch_layernorm_fwd with an fp32 branch: a bf16 branch is widened first, which is what the fused add does with it) written as
// (batch, T_out, D) fp32 tokens.  drop_cls maps the output rows onto the patch rows of [cls | patches].  The plan's backward
// buffers are free in a forward-only call: dres takes the widened branch, keep32 (read by the forward alone) the row map.
extern "C" int64_t mae_engine_tokens_workspace_bytes(const mae_engine_t* e, int32_t batch, int32_t with_cls) {
  return mae_engine_features_workspace_bytes(e, batch, with_cls);
}

extern "C" int mae_engine_extract_tokens(mae_engine_t* e, const float* params, const void* wcache, const void* images, int32_t image_dtype,
                                         int32_t batch, int32_t with_cls, int32_t drop_cls, void* workspace, int64_t workspace_bytes,
                                         float* tokens, void* stream) {
  const char* who = "mae_engine_extract_tokens";
  Plan pl;
  Ctx c{};
  MAE_TRY(begin_frozen_forward(e, params, wcache, images, image_dtype, batch, with_cls, workspace, workspace_bytes, stream, who, &pl, &c));
  MAE_REQUIRE(tokens, "%s: null argument", who);
  MAE_REQUIRE(drop_cls == 0 || (drop_cls == 1 && with_cls == 1), "%s: drop_cls = %d needs a sequence with a class row (with_cls = 1)", who, drop_cls);
  MAE_REQUIRE(e->D % 4 == 0 && e->D <= 1024, "%s: embed_dim = %d must be a multiple of 4 and at most 1024", who, e->D);
  const int T = pl.k, T_out = T - drop_cls;
  MAE_REQUIRE(T_out >= 1, "%s: no token row is left", who);
  hipStream_t s = c.s;
  c.last_block = e->depth - 1;
  MAE_TRY(run_frozen_forward(c, pl, images, image_dtype, with_cls));
  const void* branch = c.buf<>(pl.branch_b);
  if (e->act != MAE_F32) {
    MAE_TRY(launch_cast(branch, e->act, c.buf<>(pl.dres), MAE_F32, pl.Me * e->D, s));
    branch = c.buf<>(pl.dres);
  }
  const int32_t* row_map = nullptr;
  if (drop_cls) {
    MAE_TRY(launch_build_tail_row_map(batch, T, T_out, c.buf<int32_t>(pl.keep32), s));
    row_map = c.buf<int32_t>(pl.keep32);
  }
  const int64_t rows = (int64_t)batch * T_out;
  RUN(TK_LN_FWD, 0, (double)rows * e->D * 16,
      launch_layernorm_fwd(c.buf<float>(pl.enc[e->depth - 1].x_mid), branch, c.buf<float>(pl.enc_x[e->depth]), row_map, c.P(e->i_norm_w),
                           c.P(e->i_norm_b), 1e-6f, rows, e->D, MAE_F32, tokens, c.buf<float>(pl.enc_mean), c.buf<float>(pl.enc_rstd), s));
  return 0;
}

extern "C" int mae_engine_grad_sumsq_buffer(mae_engine_t* e, const float* grads, int64_t count, int32_t accumulate, float* sumsq_io,
                                            float* scratch, void* stream) {
  MAE_REQUIRE(e && grads && sumsq_io && scratch, "mae_engine_grad_sumsq_buffer: null argument");
  MAE_REQUIRE(count >= 0 && count % 4 == 0, "mae_engine_grad_sumsq_buffer: count %lld is not a multiple of 4", (long long)count);
  if (accumulate) return launch_grad_sumsq_accumulate(grads, count, sumsq_io, scratch, (hipStream_t)stream);
  return launch_grad_sumsq(grads, count, sumsq_io, scratch, (hipStream_t)stream);
}

extern "C" int mae_engine_adamw_buffer(mae_engine_t* e, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t count,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step, const float* stats,
                                       void* stream) {
  MAE_REQUIRE(e && params && grads && exp_avg && exp_avg_sq && stats, "mae_engine_adamw_buffer: null argument");
  MAE_REQUIRE(step >= 1, "mae_engine_adamw_buffer: step is 1-based");
  MAE_REQUIRE(count >= 0 && count % 4 == 0, "mae_engine_adamw_buffer: count %lld is not a multiple of 4", (long long)count);
  if (count == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const AdamBias bc = adam_bias(beta1, beta2, step);
  RUN(TK_OPTIM, 0, count * 28, launch_adamw(params, grads, exp_avg, exp_avg_sq, count, lr, beta1, beta2, eps, weight_decay, bc.c1, bc.c2, stats, nullptr, s));
  return 0;
}

extern "C" int mae_engine_refresh_transposed_range(mae_engine_t* e, const float* params, void* wcache, int64_t lo, int64_t count, void* stream) {
  MAE_REQUIRE(e && params, "mae_engine_refresh_transposed_range: null argument");
  MAE_REQUIRE(lo >= 0 && count >= 0 && lo + count <= e->trainable_elems, "mae_engine_refresh_transposed_range: range outside the trainable elements");
  if (e->act != MAE_BF16) return 0;
  MAE_REQUIRE(wcache, "mae_engine_refresh_transposed_range: null weight cache");
  hipStream_t s = (hipStream_t)stream;
  RUN(TK_OPTIM, 0, 0, refresh_transposed(e, params, wcache, s, lo, lo + count));
  return 0;
}

extern "C" int mae_engine_timers_enable(mae_engine_t* e, int32_t on) {
  MAE_REQUIRE(e, "null engine");
  e->timers_on = on != 0;
  return 0;
}
extern "C" int32_t mae_engine_timer_count(const mae_engine_t*) { return TK_COUNT; }
extern "C" const char* mae_engine_timer_name(const mae_engine_t*, int32_t kind) { return (kind >= 0 && kind < TK_COUNT) ? kTimerNames[kind] : ""; }
extern "C" int mae_engine_timers_reset(mae_engine_t* e) {
  MAE_REQUIRE(e, "null engine");
  for (auto& t : e->timers) { t.used = 0; t.flops = 0; t.bytes = 0; }
  return 0;
}
extern "C" int mae_engine_timer_read(mae_engine_t* e, int32_t kind, double* total_ms, int64_t* launches, double* flops, double* bytes) {
  MAE_REQUIRE(e && kind >= 0 && kind < TK_COUNT, "mae_engine_timer_read: bad kind");
  TimerSlot& t = e->timers[kind];
  double ms = 0;
  for (size_t i = 0; i < t.used; ++i) {
    MAE_HIP(hipEventSynchronize(t.ev[i].second));
    float f = 0;
    MAE_HIP(hipEventElapsedTime(&f, t.ev[i].first, t.ev[i].second));
    ms += f;
  }
  if (total_ms) *total_ms = ms;
  if (launches) *launches = (int64_t)t.used;
  if (flops) *flops = t.flops;
  if (bytes) *bytes = t.bytes;
  return 0;
}
