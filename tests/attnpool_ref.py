"""float64 restatement of the attentive probe (k_attnpool.hip, ssrl_vit_mae_jepa_amd/attentive.py) for the tests: the unfolded
definition (torch.float64, autograd), the folded form piece by piece as the kernels compute it (numpy float64), the launch geometry,
and per-element error bounds of the fp32 kernels.

The definition.  Tokens x (B, T, D), H heads, hd = D / H, q (D), Wk, Wv (D, D), head W (C, D), b (C):
  mu, var = per-channel mean / biased variance over all B T rows;  xh = (x - mu) rsqrt(var + eps)
  k, v = xh Wk^T, xh Wv^T;  s[b,t,h] = hd^-1/2 q[h] . k[b,t,h];  a = softmax_t s;  p[b, h hd + j] = sum_t a v[b,t,h,j]
  logits = p W^T + b;  loss = mean cross-entropy
The folded form (c = x - mu, r = rstd):
  fold         Uq[h] = r * (hd^-1/2 Wk[h]^T q[h])
  pool_fwd     s = c . Uq[h];  lse = log sum_t exp s;  a = exp(s - lse);  ybar[b,h] = sum_t a c
  project      p[b, h hd + j] = sum_d (Wv[h hd + j][d] r[d]) ybar[b,h][d]
  project_bwd  G[b,h] = r * (Wv[h]^T dp[b,h]);  dWv[h hd + j] = r * sum_b dp[b, h hd + j] ybar[b,h]
  pool_bwd     delta = ybar . G;  da = c . G;  ds = exp(s - lse) (da - delta);  dUq[h] = sum_{b,t} ds c
  fold_bwd     dU = r dUq[h];  dWk[h hd + j] = hd^-1/2 q[h hd + j] dU;  dq[h hd + j] = hd^-1/2 Wk[h hd + j] . dU
Each piece's reference takes the piece's own fp32 inputs literally (pool_bwd takes lse, ybar and G as given), so no bound has to carry
another kernel's error.

Geometry.  A lane holds the float4 columns lane + 64 i, i < NV = ceil(D / 256).  HG = 1 / 2 / 4 head groups for H <= 4 / 8 / 16,
HPW = ceil(H / HG) heads per wave, TS = 4 / HG waves split the tokens of a head group in chunks of TC rows (forward 4, backward 2):
a wave walks NCH = ceil(T / (TC TS)) chunks at most.  The backward gives IPB = ceil(B / 512) consecutive images to a block,
GRID = ceil(B / IPB) blocks, whose partials sum_partials (k_patch.hip) adds: ceil(GRID / 32) strided, then 32 serial additions.

Bounds.  u = 2^-24; every fp32 operation returns x (1 + d), |d| <= u; a term that went through k of them is off by at most k u of its
size to first order, SECOND = 1 + 2^-16 covers the second order (every k here stays below 1200).  Fused multiply-adds only remove
roundings.  expf and logf are taken within EXP_ULP = 2 ulp = 4 u.  A dot product over D by this layout is a chain of 4 NV fused
multiply-adds per lane and 6 butterfly additions: kd = 4 NV + 6; the small kernels walk four float4 per lane whatever D is: kd4 = 22.
  c       fl(x - mu): 1 (0 without a mean, where c = x exactly)                                                          kc = 0 | 1
  s       |err| <= (kd + kc) u sum_d |c Uq|                                                                              =: bs[b,t,h]
  weights the kernel's weight of token t is exp(s - M) (1 + e_t), the SAME float in the numerator and in the denominator of ybar: the
          score's error bs, the rounding of the exponent's argument (u |s - m| <= u range, range = max_t s - min_t s + 1), expf; then
          NCH - 1 rescales and the merge, each one expf of a rounded difference of maxima, and the differences add up to at most
          range each time:    e_t = expm1(bs + u (EXP (NCH + 1) + 3 range))
  ybar    with A = sum_t a |c|, E = sum_t a e_t |c|, ebar = sum_t a e_t: the weights move ybar by (E + |ybar| ebar) / (1 - ebar);
          a numerator term goes through c, its fused add, TC NCH - 1 later additions, NCH rescales, TS products and TS additions of the
          merge and the division: kN = kc + TC NCH + NCH + 2 TS + 1; the denominator the same without c: kL = kN - kc, relative.
          A weight below 2^-126 is flushed: T 2^-125 max_t |c| more.
                                       |err| <= (E + |ybar| ebar) / (1 - ebar) + (kN + kL) u A + T 2^-125 max|c|
  lse     fl(M + logf(L)): log L moves by ebar / (1 - ebar) + kL u, logf rounds log L <= log T + 1 within EXP, the addition rounds lse
                                       |err| <= ebar / (1 - ebar) + kL u + EXP u (log T + 1) + u |lse|
  pool_bwd  a^ = expf(fl(s^ - lse)) = a (1 + ea), ea = expm1(bs + u (|s - lse| + EXP)); da and delta are dot products: bda =
          (kd + kc) u sum |c G|, bdl = kd u sum |ybar G|; the difference rounds once, the product with a^ once:
          bds = a (1 + ea) (bda + bdl + u |da - delta|) + |ds| (ea + u).  A term ds c then carries kc and goes through
          kA = IPB TC NCH + TS + ceil(GRID / 32) + 32 additions:
                                       |err| <= sum_{b,t} bds |c| + (kA + kc) u sum_{b,t} |ds c|
  fold    hd fused additions in order, hd^-1/2 = fl(1 / sqrtf(hd)) (2), its product, the product with r:
                                       |err| <= (hd + 4) u |r| hd^-1/2 sum_j |q Wk|
  project fl(Wv r) (1) then kd4:       |err| <= (kd4 + 1) u sum_d |Wv r ybar|
  G       hd additions, the product with r:                              |err| <= (hd + 1) u |r| sum_j |dp Wv|
  dWv     per_slice = ceil(B / min(ceil(B / 64), 8)) additions in a slice, sum_partials over at most 8 slices (1 + 32), r:
                                       |err| <= (per_slice + 34) u |r| sum_b |dp ybar|
  dWk     fl(r dUq) (1), fl(fl(hd^-1/2) q) (3), the product (1):          |err| <= 5 u |dWk|
  dq      fl(r dUq) (1), kd4, hd^-1/2 (2) and its product (1):            |err| <= (kd4 + 4) u hd^-1/2 sum_d |Wk r dUq|
Bounds are evaluated from the inputs and the float64 reference only.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16
EXP_ULP = 2
EXP = 2.0 * EXP_ULP          # in units of u
FWD_TC, BWD_TC, BWD_SLOTS, SP_LANES, WV_SLICES = 4, 2, 512, 32, 8
KD4 = 22
F = np.float32


def f32(x) -> float:
    return float(F(x))


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _d(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ geometry
def geometry(D: int, H: int, T: int = 1, B: int = 1) -> dict:
    assert D % 4 == 0 and 4 <= D <= 1024 and 1 <= H <= 16 and D % H == 0 and T >= 1 and B >= 1
    nv = cdiv(D // 4, 64)
    hg = 1 if H <= 4 else 2 if H <= 8 else 4
    ts = 4 // hg
    ipb = cdiv(B, BWD_SLOTS)
    grid = cdiv(B, ipb)
    return dict(nv=nv, hg=hg, hpw=cdiv(H, hg), ts=ts, kd=4 * nv + 6, nch_fwd=cdiv(T, FWD_TC * ts), nch_bwd=cdiv(T, BWD_TC * ts), ipb=ipb, grid=grid,
                bwd_scratch_bytes=grid * H * D * 4, wv_slices=min(cdiv(B, 64), WV_SLICES))


# ------------------------------------------------------------------------------------------------ the definition, torch fp64
def definition(x, q, wk, wv, w, b, labels, H: int, eps: float = 1e-6, stats=None) -> dict:
    """The unfolded definition with autograd: dict(p, logits, loss, mu, var, dq, dwk, dwv, dw, db), numpy float64.  stats = (mean, var):
    the evaluation form with those statistics instead of the batch's."""
    dt = torch.float64
    x = torch.as_tensor(np.asarray(x), dtype=dt)
    q, wk, wv, w, b = (torch.as_tensor(np.asarray(t), dtype=dt).clone().requires_grad_() for t in (q, wk, wv, w, b))
    B, T, D = x.shape
    hd = D // H
    if stats is None:
        mu, var = x.reshape(-1, D).mean(0), x.reshape(-1, D).var(0, unbiased=False)
    else:
        mu, var = (torch.as_tensor(np.asarray(t), dtype=dt) for t in stats)
    xh = (x - mu) * (var + f32(eps)).rsqrt()
    k = (xh @ wk.T).reshape(B, T, H, hd)
    v = (xh @ wv.T).reshape(B, T, H, hd)
    s = torch.einsum("hj,bthj->bth", q.reshape(H, hd), k) * hd ** -0.5
    a = s.softmax(1)
    p = torch.einsum("bth,bthj->bhj", a, v).reshape(B, D)
    logits = p @ w.T + b
    out = dict(p=p, logits=logits, mu=mu, var=var, a=a)
    if labels is not None:
        loss = torch.nn.functional.cross_entropy(logits, torch.as_tensor(np.asarray(labels), dtype=torch.int64))
        g = torch.autograd.grad(loss, [q, wk, wv, w, b])
        out.update(loss=loss, dq=g[0], dwk=g[1], dwv=g[2], dw=g[3], db=g[4])
    return {k_: v_.detach().numpy() for k_, v_ in out.items()}


# ------------------------------------------------------------------------------------------------ the folded pieces, numpy fp64
def fold(q, wk, rstd, H: int) -> np.ndarray:
    q, wk, rstd = _d(q), _d(wk), _d(rstd)
    D = q.size
    hd = D // H
    return rstd * hd ** -0.5 * np.einsum("hj,hjd->hd", q.reshape(H, hd), wk.reshape(H, hd, D))


def pool_fwd(x, mean, uq) -> dict:
    """dict(c, s, lse, a, ybar)."""
    c = _d(x) - (0.0 if mean is None else _d(mean))
    s = np.einsum("btd,hd->bth", c, _d(uq))
    m = s.max(1, keepdims=True)
    lse = (m + np.log(np.exp(s - m).sum(1, keepdims=True)))[:, 0]
    a = np.exp(s - lse[:, None])
    return dict(c=c, s=s, lse=lse, a=a, ybar=np.einsum("bth,btd->bhd", a, c))


def project(ybar, rstd, wv, H: int) -> np.ndarray:
    ybar, rstd, wv = _d(ybar), _d(rstd), _d(wv)
    B, _, D = ybar.shape
    return np.einsum("bhd,hjd->bhj", ybar * rstd, wv.reshape(H, D // H, D)).reshape(B, D)


def project_bwd(dp, ybar, rstd, wv, H: int) -> dict:
    """dict(g (B, H, D), dwv (D, D))."""
    dp, ybar, rstd, wv = _d(dp), _d(ybar), _d(rstd), _d(wv)
    B, _, D = ybar.shape
    dph = dp.reshape(B, H, D // H)
    return dict(g=rstd * np.einsum("bhj,hjd->bhd", dph, wv.reshape(H, D // H, D)),
                dwv=(rstd * np.einsum("bhj,bhd->hjd", dph, ybar)).reshape(D, D))


def pool_bwd(x, mean, uq, lse, ybar, g) -> dict:
    """dict(c, s, a, da, delta, ds, duq) from the inputs as given."""
    c = _d(x) - (0.0 if mean is None else _d(mean))
    s = np.einsum("btd,hd->bth", c, _d(uq))
    a = np.exp(s - _d(lse)[:, None])
    da = np.einsum("btd,bhd->bth", c, _d(g))
    delta = (_d(ybar) * _d(g)).sum(-1)
    ds = a * (da - delta[:, None])
    return dict(c=c, s=s, a=a, da=da, delta=delta, ds=ds, duq=np.einsum("bth,btd->hd", ds, c))


def fold_bwd(duq, q, wk, rstd, H: int) -> dict:
    """dict(dq (D), dwk (D, D))."""
    duq, q, wk, rstd = _d(duq), _d(q), _d(wk), _d(rstd)
    D = q.size
    hd = D // H
    du = rstd * duq
    return dict(dwk=(hd ** -0.5 * np.einsum("hj,hd->hjd", q.reshape(H, hd), du)).reshape(D, D),
                dq=(hd ** -0.5 * np.einsum("hjd,hd->hj", wk.reshape(H, hd, D), du)).reshape(D))


def head(p, w, b, labels) -> dict:
    """logits, mean cross-entropy, dp, dW, db of the linear head on p."""
    p, w, b = _d(p), _d(w), _d(b)
    logits = p @ w.T + b
    z = logits - logits.max(1, keepdims=True)
    logp = z - np.log(np.exp(z).sum(1, keepdims=True))
    n = p.shape[0]
    lab = np.asarray(labels, dtype=np.int64)
    dl = np.exp(logp)
    dl[np.arange(n), lab] -= 1.0
    dl /= n
    return dict(logits=logits, loss=float(-logp[np.arange(n), lab].mean()), correct=int((logits.argmax(1) == lab).sum()), dp=dl @ w, dw=dl.T @ p,
                db=dl.sum(0))


def folded(x, q, wk, wv, w, b, labels, H: int, eps: float = 1e-6, stats=None) -> dict:
    """The whole step in the folded form: the pieces above chained in float64."""
    x = _d(x)
    B, T, D = x.shape
    if stats is None:
        mu = x.reshape(-1, D).mean(0)
        var = ((x.reshape(-1, D) - mu) ** 2).mean(0)
    else:
        mu, var = _d(stats[0]), _d(stats[1])
    rstd = 1.0 / np.sqrt(var + f32(eps))
    uq = fold(q, wk, rstd, H)
    f = pool_fwd(x, mu, uq)
    p = project(f["ybar"], rstd, wv, H)
    h = head(p, w, b, labels)
    pb = project_bwd(h["dp"], f["ybar"], rstd, wv, H)
    bw = pool_bwd(x, mu, uq, f["lse"], f["ybar"], pb["g"])
    fb = fold_bwd(bw["duq"], q, wk, rstd, H)
    return dict(mu=mu, var=var, rstd=rstd, uq=uq, lse=f["lse"], ybar=f["ybar"], a=f["a"], p=p, logits=h["logits"], loss=h["loss"], dp=h["dp"],
                g=pb["g"], ds=bw["ds"], duq=bw["duq"], dq=fb["dq"], dwk=fb["dwk"], dwv=pb["dwv"], dw=h["dw"], db=h["db"])


# ------------------------------------------------------------------------------------------------ bounds
def pool_fwd_bounds(ref: dict, uq, has_mean: bool, H: int) -> dict:
    """dict(ybar, lse) of bounds for pool_fwd's ref."""
    c, s, a = ref["c"], ref["s"], ref["a"]
    B, T, D = c.shape
    g = geometry(D, H, T, B)
    kc = 1 if has_mean else 0
    ac = np.abs(c)
    bs = SECOND * (g["kd"] + kc) * U * np.einsum("btd,hd->bth", ac, np.abs(_d(uq)))
    rng = s.max(1) - s.min(1) + 1.0                                                  # (B, H)
    e = np.expm1(SECOND * (bs + U * (EXP * (g["nch_fwd"] + 1) + 3.0 * rng[:, None])))  # (B, T, H)
    A = np.einsum("bth,btd->bhd", a, ac)
    E = np.einsum("bth,btd->bhd", a * e, ac)
    ebar = (a * e).sum(1)                                                            # (B, H)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(ebar < 1.0, 1.0 / (1.0 - ebar), np.inf)
    kN = kc + FWD_TC * g["nch_fwd"] + g["nch_fwd"] + 2 * g["ts"] + 1
    kL = kN - kc
    ybar = SECOND * ((E + np.abs(ref["ybar"]) * ebar[..., None]) * inv[..., None] + (kN + kL) * U * A) + T * 2.0 ** -125 * ac.max(1)[:, None, :]
    lse = SECOND * (ebar * inv + kL * U + EXP * U * (math.log(T) + 1.0) + U * np.abs(ref["lse"]))
    return dict(ybar=ybar, lse=lse, bs=bs)


def pool_bwd_bounds(ref: dict, uq, lse, ybar, g, has_mean: bool, H: int) -> np.ndarray:
    """Bound of duq (H, D) for pool_bwd's ref."""
    c, s, a, ds = ref["c"], ref["s"], ref["a"], ref["ds"]
    B, T, D = c.shape
    geo = geometry(D, H, T, B)
    kc = 1 if has_mean else 0
    ac = np.abs(c)
    bs = (geo["kd"] + kc) * U * np.einsum("btd,hd->bth", ac, np.abs(_d(uq)))
    ea = np.expm1(SECOND * (bs + U * (np.abs(s - _d(lse)[:, None]) + EXP)))
    bda = (geo["kd"] + kc) * U * np.einsum("btd,bhd->bth", ac, np.abs(_d(g)))
    bdl = geo["kd"] * U * (np.abs(_d(ybar)) * np.abs(_d(g))).sum(-1)
    bds = a * (1.0 + ea) * (bda + bdl[:, None] + U * np.abs(ref["da"] - ref["delta"][:, None])) + np.abs(ds) * (ea + U)
    kA = geo["ipb"] * BWD_TC * geo["nch_bwd"] + geo["ts"] + cdiv(geo["grid"], SP_LANES) + SP_LANES
    return SECOND * (np.einsum("bth,btd->hd", bds, ac) + (kA + kc) * U * np.einsum("bth,btd->hd", np.abs(ds), ac))


def fold_bound(q, wk, rstd, H: int) -> np.ndarray:
    q, wk, rstd = np.abs(_d(q)), np.abs(_d(wk)), np.abs(_d(rstd))
    D = q.size
    hd = D // H
    return SECOND * (hd + 4) * U * rstd * hd ** -0.5 * np.einsum("hj,hjd->hd", q.reshape(H, hd), wk.reshape(H, hd, D))


def project_bound(ybar, rstd, wv, H: int) -> np.ndarray:
    return SECOND * (KD4 + 1) * U * project(np.abs(_d(ybar)), np.abs(_d(rstd)), np.abs(_d(wv)), H)


def project_bwd_bounds(dp, ybar, rstd, wv, H: int) -> dict:
    B, _, D = np.shape(ybar)
    hd = D // H
    m = project_bwd(np.abs(_d(dp)), np.abs(_d(ybar)), np.abs(_d(rstd)), np.abs(_d(wv)), H)
    slices = min(cdiv(B, 64), WV_SLICES)
    return dict(g=SECOND * (hd + 1) * U * m["g"], dwv=SECOND * (cdiv(B, slices) + 34) * U * m["dwv"])


def fold_bwd_bounds(duq, q, wk, rstd, H: int) -> dict:
    m = fold_bwd(np.abs(_d(duq)), np.abs(_d(q)), np.abs(_d(wk)), np.abs(_d(rstd)), H)
    return dict(dwk=SECOND * 5 * U * m["dwk"], dq=SECOND * (KD4 + 4) * U * m["dq"])


# ------------------------------------------------------------------------------------------------ data
T_LIST = [1, 2, 63, 64, 65, 144, 145, 257]
DH_LIST = [(64, 1), (64, 4), (100, 5), (192, 3), (384, 6), (1024, 16)]
MANY_IMAGES = 2 * BWD_SLOTS + 3      # more images than the backward has partial slots: two or three images a block, the last block short


def kernel_cases():
    """(B, T, D, H): every T at (384, 6), every (D, H) at T = 145, B alternating 1 and 3, and the many-image case."""
    out = []
    for i, T in enumerate(T_LIST):
        out.append((1 + 2 * (i % 2), T, 384, 6))
    for i, (D, H) in enumerate(DH_LIST):
        if (D, H) != (384, 6):
            out.append((3 - 2 * (i % 2), 145, D, H))
    out.append((MANY_IMAGES, 2, 64, 4))
    return out


def gen_case(B: int, T: int, D: int, H: int, seed: int = 0, score_scale: float = 1.0) -> dict:
    """fp32 inputs of one shape: tokens that look like LayerNorm output (column means spread over +-2, spreads over [0.3, 2]), their
    statistics, probe weights large enough for a peaked softmax, a gradient dp of a head's size."""
    r = np.random.default_rng([B, T, D, H, seed])
    means = r.permutation(np.linspace(-2.0, 2.0, D))
    stds = r.permutation(np.geomspace(0.3, 2.0, D))
    x = (means + stds * r.standard_normal((B, T, D))).astype(F)
    flat = x.reshape(-1, D).astype(np.float64)
    mean = flat.mean(0).astype(F)
    rstd = (1.0 / np.sqrt(flat.var(0) + 1e-6)).astype(F) if B * T > 1 else np.ones(D, dtype=F)
    q = (score_scale * r.standard_normal(D)).astype(F)
    wk = (r.standard_normal((D, D)) * (4.0 / math.sqrt(D))).astype(F)
    wv = (r.standard_normal((D, D)) / math.sqrt(D)).astype(F)
    dp = (r.standard_normal((B, D)) * 1e-2).astype(F)
    return dict(x=x, mean=mean, rstd=rstd, q=q, wk=wk, wv=wv, dp=dp)


# ------------------------------------------------------------------------------------------------ comparison
def worst(out, ref, bound):
    """(worst error / bound, flat index of it); an element that is not finite, or off where the bound is zero, counts as infinite."""
    err = np.abs(_d(out) - _d(ref))
    bound = np.broadcast_to(_d(bound), err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), i
