"""Reference, bound, case table and oracle walk for the attention-map kernel (k_attnmap.hip: attn_colsum_kernel) and the engine call
built on it (mae_engine_extract_attention).

Torch only (no HIP library): tests/test_attnmap_ref_host.py runs it on the CPU, the GPU tests where the tensors live.

Layout: qkv (B, T, 3 H hd) as tests/attn_ref.py; w (B, T); per_head (B, H, T); mixed (B, T).  Per head, P (B, H, T, T) [query t, key j].

Reference (fp64, from the operand values as stored, scale = hd^-1/2 in fp64):
  S = scale Q K^T, P = softmax_j S, per_head[b,h,j] = sum_t w[b,t] P[b,h,t,j], mixed = w / 2 + mean_h per_head / 2
  rollout = w A_top ... A_0 with A_l = (mean_h P_l + I) / 2, evaluated as the chain r <- mixed(r) from the top block downwards;
  rollout_matrix forms the explicit product, for the test that the two agree.

Bound of the fp32 kernel against that reference, first order, per element.  u = 2^-24 (unit roundoff of fp32), E_EXP of attn_ref
(1 ulp of the result of v_exp_f32 = 2 u), A_tj = scale sum_d |q_td k_jd|, X_tj = |S_tj - M_t| (M_t = max_j S_tj), absw = |w|.
Read off the kernel's statements:
  score   s_tj: hd fused multiply-adds over d in index order from 0 (hd roundings, each at most u times the partial sum of absolute
          products <= u A_tj / scale), then one product with scale = 1 / sqrtf(hd) (the square root, the division, the product:
          3 u |S_tj| <= 3 u A_tj):                                               eS_tj = (hd + 3) u A_tj                    [nats]
  shift   x = s - m: m is the same float for every key of the row, so it cancels between a term and the row's sum whatever its own
          error; the subtraction rounds once (u X), and __expf multiplies by a rounded log2 e (u X) and rounds that product (u X):
          3 u X_tj nats.  (Fused into one multiply-add by the compiler, the product with scale is not rounded and x has one rounding:
          less, never more.)
  exp     e_tj = v_exp_f32(...): relative E_EXP.        =>  relative error of e_tj:   eE_tj = eS_tj + 3 u X_tj + E_EXP
  sum     l_t = sum_j e_tj: a lane adds its NK = ceil(T / 64) keys in order (NK - 1 roundings after the first), the butterfly adds
          6 levels; every term passes through at most NK + 5 roundings of partial sums that never exceed l_t (all terms >= 0), and
          carries its own eE:                                                    eL_t = sum_j P_tj eE_tj + (NK + 5) u
  coef    w_t / l_t: one division, 1 u when correctly rounded; 2 u allowed.
  column  acc_j += coef e_tj by one fused multiply-add per row a wave owns -- groups of ROWS = 4 consecutive rows dealt to WAVES = 4
          waves, ROWS ceil(T / 16) rows at most -- then the four waves' sums are added in three roundings: every rounding is at most
          u times a partial sum of absolute terms <= sum_t absw_t P_tj:          c_sum = 4 ceil(T / 16) + 3
  =>  e_head[b,h,j] = SECOND sum_t absw_t P_tj (eE_tj + eL_t + 2 u) + c_sum u sum_t absw_t P_tj + TINY (1 + sum_t absw_t)
      SECOND = 1 + 4 * 2^-8 covers products of two first-order terms as in attn_ref; TINY (2^-120) sum absw covers exponentials
      that v_exp_f32 flushes to zero below the normal range, and the lone TINY keeps the bound of an all-zero weight row positive.
  mixed   hsum = sum_h per_head in head order (H - 1 roundings), (1 / 2) / H rounded once on the host, one fused multiply-add with
          the exact w / 2:
      e_mixed[b,j] = sum_h e_head[b,h,j] / (2 H) + (H + 1) u sum_h absS[b,h,j] / (2 H) + u |mixed_ref[b,j]|,  absS = sum_t absw P.
bf16 operands are widened exactly, so both activation types share the bound.  None of the constants comes from a run.
"""
from __future__ import annotations

import dataclasses
import itertools
import math
from functools import lru_cache

import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests.attn_ref import E_EXP, HDS, SECOND, TINY, U32, split_heads

TS = (1, 2, 17, 63, 64, 65, 128, 129, 145, 197, 257)   # the lengths of the issue; cases() adds the kernel's limit
HEADS = (1, 2, 3, 6, 16)
BATCHES = (1, 3, 7)
DTYPES = ("f32", "bf16")
WAVES, ROWS = 4, 4                                      # AC_WAVES, AC_ROWS of k_attnmap.hip
WEIGHTS = ("onehot_first", "onehot_last", "uniform", "sparse", "chained")


# ------------------------------------------------------------------------------------------------ reference
def probabilities(qkv, H, hd):
    """-> S, P (B, H, T, T) fp64 and A = scale |Q| |K|^T, from the stored operand values."""
    q, k, _ = (x.double() for x in split_heads(qkv, H, hd, 3))
    scale = hd ** -0.5
    S = scale * (q @ k.transpose(-1, -2))
    E = torch.exp(S - S.amax(-1, keepdim=True))
    return S, E / E.sum(-1, keepdim=True), scale * (q.abs() @ k.abs().transpose(-1, -2))


def colsum_from(P, w):
    return torch.einsum("bt,bhtj->bhj", w.double(), P)


def colsum_ref(qkv, w, H, hd):
    """per_head (B, H, T) fp64."""
    return colsum_from(probabilities(qkv, H, hd)[1], w)


def mixed_ref(w, per_head):
    """(B, T) fp64: one rollout step from the per-head column sums."""
    return 0.5 * w.double() + 0.5 * per_head.double().mean(1)


def rollout_ref(Ps, w, top=None):
    """Ps: every block's P (B, H, T, T), block 0 first.  The chain from block `top` (default the last) down to block 0."""
    top = len(Ps) - 1 if top is None else top
    r = w.double()
    for l in range(top, -1, -1):
        r = mixed_ref(r, colsum_from(Ps[l].double(), r))
    return r


def rollout_matrix(Ps, top=None):
    """The explicit product A_top ... A_0 (B, T, T), A_l = (mean_h P_l + I) / 2."""
    top = len(Ps) - 1 if top is None else top
    T = Ps[0].shape[-1]
    eye = torch.eye(T, dtype=torch.float64, device=Ps[0].device)
    out = None
    for l in range(top, -1, -1):
        A = 0.5 * Ps[l].double().mean(1) + 0.5 * eye
        out = A if out is None else out @ A
    return out


# ------------------------------------------------------------------------------------------------ bound
def colsum_bound(qkv, w, H, hd, parts=None):
    """-> e_head (B, H, T), e_mixed (B, T), fp64 (module docstring).  parts: probabilities(qkv, H, hd), when the caller has them."""
    S, P, A = probabilities(qkv, H, hd) if parts is None else parts
    T = S.shape[-1]
    nk = -(-T // 64)
    X = (S - S.amax(-1, keepdim=True)).abs()
    eE = (hd + 3) * U32 * A + 3 * U32 * X + E_EXP
    eL = (P * eE).sum(-1) + (nk + 5) * U32                       # (B, H, T)
    aw = w.double().abs()
    absS = torch.einsum("bt,bhtj->bhj", aw, P)
    e_head = (SECOND * torch.einsum("bt,bhtj->bhj", aw, P * (eE + eL[..., None] + 2 * U32)) + (ROWS * -(-T // (ROWS * WAVES)) + 3) * U32 * absS
              + TINY * (1 + aw.sum(-1))[:, None, None])
    ref_mixed = mixed_ref(w, colsum_from(P, w))
    e_mixed = e_head.sum(1) / (2 * H) + (H + 1) * U32 * absS.sum(1) / (2 * H) + U32 * ref_mixed.abs()
    return e_head, e_mixed


# ------------------------------------------------------------------------------------------------ cases and inputs
@dataclasses.dataclass(frozen=True)
class Case:
    dtype: str
    B: int
    T: int
    H: int
    hd: int

    @property
    def id(self):
        return f"{self.dtype}-B{self.B}-T{self.T}-H{self.H}-hd{self.hd}"

    @property
    def route(self):
        """The kernel instance: the activation type and NK, the key registers of a lane (1, 2, 3, 4, 5, or 8 beyond)."""
        nk = -(-self.T // 64)
        return f"{self.dtype}/NK{nk if nk <= 5 else 8}"


PAIRS = (("T", "dtype"), ("hd", "H"), ("hd", "B"), ("hd", "dtype"), ("H", "B"), ("H", "dtype"), ("B", "dtype"))


def uncovered(table, max_tokens):
    """The value pairs of PAIRS that no case of the table holds."""
    dom = dict(T=TS + (max_tokens,), hd=HDS, H=HEADS, B=BATCHES, dtype=DTYPES)
    return [(a, b, va, vb) for a, b in PAIRS for va in dom[a] for vb in dom[b]
            if not any(getattr(c, a) == va and getattr(c, b) == vb for c in table)]


@lru_cache(None)
def cases(max_tokens=512):
    """Every length with three of the five head widths (each width with 7 or 8 of the 12 lengths), the other parameters chosen greedily in
    a fixed order so that every pair of PAIRS occurs: 36 cases, not the 1800 of the full product.  The largest images (7 x 16 heads)
    are kept off the longest sequence, whose fp64 reference is 8 T^2 bytes per head."""
    dom = dict(T=TS + (max_tokens,), hd=HDS, H=HEADS, B=BATCHES, dtype=DTYPES)
    need = {(a, b, va, vb) for a, b in PAIRS for va in dom[a] for vb in dom[b]}
    out = []
    for T, hd in ((T, HDS[(i + 2 * k) % 5]) for i, T in enumerate(dom["T"]) for k in range(3)):
        best, gain, n = None, -1, len(out)
        rot = lambda v, s: v[s % len(v):] + v[:s % len(v)]   # noqa: E731  (ties go to a different value in every case)
        for H, B, dt in itertools.product(rot(HEADS, n), rot(BATCHES, n), rot(DTYPES, n)):
            if T == max_tokens and B * H > 48:
                continue
            c = Case(dt, B, T, H, hd)
            g = sum((a, b, getattr(c, a), getattr(c, b)) in need for a, b in PAIRS)
            if g > gain:
                best, gain = c, g
        out.append(best)
        need -= {(a, b, getattr(best, a), getattr(best, b)) for a, b in PAIRS}
    return tuple(out)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % 2147483647
    return torch.Generator().manual_seed(seed)


def gen_qkv(c: Case, family, dtype):
    """family "random": sigma = 1.  "large": q and k at sigma = 16, so that the scaled scores have a spread of 256 and exceed +-100
    in every row of more than a few keys: exp of an unshifted score overflows."""
    g = _gen(7, c.B, c.T, c.H, c.hd, 0 if family == "random" else 1)
    x = torch.randn(c.B, c.T, 3 * c.H * c.hd, generator=g)
    if family == "large":
        x = x * 16.0
    return x.to(dtype)


def gen_weights(c: Case):
    """The start weights of a case, (B, T) fp32, by name; "chained" is made by the caller from a previous call's mixed."""
    g = _gen(9, c.B, c.T, c.H, c.hd)
    first = torch.zeros(c.B, c.T)
    first[:, 0] = 1.0
    last = torch.zeros(c.B, c.T)
    last[:, c.T - 1] = 1.0
    sparse = torch.rand(c.B, c.T, generator=g) * (torch.rand(c.B, c.T, generator=g) < 0.6)
    sparse[:, c.T // 2] = 0.0                                   # an exact zero in every image, whatever the draw
    if c.T >= 2:
        sparse[:, 0] = 0.25
    return {"onehot_first": first, "onehot_last": last, "uniform": torch.full((c.B, c.T), 1.0 / c.T), "sparse": sparse}


# ------------------------------------------------------------------------------------------------ oracle walk
def oracle_walk(params, cfg, images, with_cls=True, bf16=False):
    """Every encoder block's attention probabilities (B, H, T, T), block 0 first, from the oracle's own pieces: the embedding of
    forward_encoder, and per block the LayerNorm, the qkv Linear and its rounding, the scaled softmax of _attention, then _block for the
    residual stream.  Precision follows the parameters: fp32, fp32 with bf16=True (the bf16 emulation), or fp64 parameters and images
    with bf16=False."""
    B = images.shape[0]
    H, D = cfg.num_heads, cfg.embed_dim
    hd = D // H
    tok = O.patch_embed_all(images, params, cfg, bf16)
    pos = params["encoder.vit.pos_embed"]
    if with_cls:
        tok = torch.cat([params["encoder.vit.cls_token"].expand(B, -1, -1), tok], dim=1) + pos
    else:
        tok = tok + pos[:, 1:]
    out = []
    for i in range(cfg.depth):
        pfx = f"encoder.vit.blocks.{i}"
        h = F.layer_norm(tok, (D,), params[f"{pfx}.norm1.weight"], params[f"{pfx}.norm1.bias"], O.LN_EPS)
        qkv = O._r(O._linear(h, params[f"{pfx}.attn.qkv.weight"], params[f"{pfx}.attn.qkv.bias"], bf16), bf16)
        q, k, _ = qkv.reshape(B, -1, 3, H, hd).permute(2, 0, 3, 1, 4).unbind(0)
        out.append(((q * hd ** -0.5) @ k.transpose(-2, -1)).softmax(dim=-1))
        tok = O._block(tok, params, pfx, H, bf16)
    return out


def walk_fp64(params, cfg, images, with_cls=True):
    return oracle_walk({k: v.double() for k, v in params.items()}, cfg, images.double(), with_cls, False)


def start_weight(query, B, T, dtype=torch.float64):
    w = torch.zeros(B, T, dtype=dtype)
    if query == "cls":
        w[:, 0] = 1.0
    else:
        w[:] = 1.0 / T
    return w


def maps_of(Ps, query, layers):
    """(B, n, H, T) fp64: what extract_attention returns for `layers`, from a walk's probabilities."""
    B, _, T, _ = Ps[0].shape
    w = start_weight(query, B, T)
    return torch.stack([colsum_from(Ps[l].double(), w) for l in layers], dim=1)
