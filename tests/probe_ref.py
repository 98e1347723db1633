"""float64 restatement of the linear probe (k_probe.hip, ssrl_vit_mae_jepa_amd/probe.py) for the tests, the launch geometry of its two
kernels, and per-element error bounds of the fp32 kernels.

numpy on the CPU, float64 throughout.  Hyperparameters enter as the fp32 values the C ABI receives, widened to double (``f32``).

  bn_train    torch.nn.BatchNorm1d(dim, affine=False, eps) in train mode: biased variance in y, unbiased in running_var
  bn_eval     the same in eval mode: y = (x - running_mean) / sqrt(running_var + eps)
  lars_step   the LARS of the MAE code base: dp = g + wd p, q = tc |p| / |dp| (1 where a norm is 0), dp q; 1-D tensors (adapt = 0): dp = g;
              mu' = momentum mu + dp, p' = p - lr mu'
  fold        BatchNorm's eval form folded into the linear layer
  probe_step  bn_train -> logits, mean cross-entropy, dW, db -> lars_step on W (adapt 1) and on b (adapt 0)

Geometry of mae_batchnorm_fwd (training).  d4 = dim / 4; a block covers RP = 256 // d4 rows per trip; G blocks own contiguous slices of
S rows (S a multiple of RP, want = min(ceil(rows / 4 RP), 1024), S = round_up(ceil(rows / want), RP), G = ceil(rows / S)) and make
T = S / RP trips.  A thread adds one term per trip, the RP row slots of a block are added in order through LDS, sum_partials (k_patch.hip)
adds the G partial rows: row lane rl adds rows rl, rl + 32, .. in order, then the 32 row lanes are added in order.

Bounds.  u = 2^-24; every fp32 operation returns x (1 + d), |d| <= u, division and square root included; a value that went through k of
them is off by at most k u to first order; the second-order terms are about k u / 2 of that, and every k here stays below 400 (the most
is dim 4 with its 256 row slots), so SECOND = 1 + 2^-16 covers them.  Fused multiply-adds (-ffp-contract=fast) only remove roundings.  All counts need normal numbers or exact
zeros.  tail = T + RP + ceil(G / 32) + 32: the per-trip `+=`, the LDS stage, the strided and the serial sums of the second stage.
  mean   the kernel sums fl(x - x0) about the pivot row x0 = x[0]: the difference 1, then tail          k0 = 1 + tail
         mean = fl(x0 + fl(S0 / fl(rows))): fl(rows) and the division 2 more on the sum, the last addition rounds |mean| once
                                                   |err| <= (k0 + 2) u sum_r |x - x0| / rows + u |mean|                         =: bm
  var    the kernel sums (x - m)^2 about its own mean m = mean + e, which is rows (var + e^2) exactly.  fl(x - m) = 1, squared = 2,
         the product = 1, then tail:               k2 = 3 + tail;   var = fl(M2 / fl(rows)) = 2 more
                                                   |err| <= (k2 + 2) u (var + bm^2) + bm^2                                      =: bv
  rstd   fl(var + eps) = 1 on a positive sum, halved by the power -1/2, and rsqrtf within RSQRT_ULP = 2 ulp = 4 u (as tests/ln_ref.py
         allows it).  t = bv / (var + eps) + u:       rel = t (1 + t) / 2 + 4 u
  y      fl(fl(x - m) rstd), a = (x - mean) rstd: the subtraction carries bm and 1, rstd rel, the product 1
                                                   |err| <= rstd bm + |a| (rel + 2 u)
  running_mean'  fl(fl(rm keep) + fl(m mom)), keep = fl(1 - mom): keep, product, sum = 3 on |(1 - mom) rm|; product, sum = 2 on |mom mean|
                                                   |err| <= 3 u |(1 - mom) rm| + 2 u |mom mean| + mom bm
  running_var'   unb = fl(M2 / fl(rows - 1)): M2 is off by rows ((k2 u)(var + bm^2) + bm^2) =: bM2, the conversion and division 2
                                                   |err| <= 3 u |(1 - mom) rv| + 2 u |mom unb| + mom (bM2 / (rows - 1) + 2 u unb)
  evaluation     rstd = rsqrtf(fl(rv + eps)): t = u;  y = fl(fl(x - rm) rstd), a = (x - rm) rstd:     |err| <= |a| (rel + 2 u)

mae_lars_step.  lars_sumsq_kernel is sumsq_kernel (k_loss_optim.hip) with two accumulators, so tests/optim_ref.py's chain holds:
k = I + F + 22, I = ceil((n / 4) / (grid 256)), grid = min(ceil(n / 1024), 1024), F = ceil(grid / 256).
  pn     |p| = fl(sqrt(sum p^2)), exact squares of the inputs:                          rel_pn = (k / 2 + 1) u
  un     the kernel squares its own dp^ = fl(g + fl(wd p)), off by e = 2 u (|g| + |wd p|) per element, so | |dp^| - |dp| | <= |e|_2:
                                                   |err| <= |e|_2 + (k / 2 + 1) u (un + |e|_2)                                  =: bun
  q      fl(fl(tc pn) / un), r = bun / un:          rel_q = (rel_pn + 2 u + r) / (1 - r)
  d      fl(dp^ q^), d = dp q:                      |err| <= q (1 + rel_q) e + |d| (rel_q + u)                                   =: bd
         adapt = 0: d = g exactly, bd = 0
  mu'    fl(fl(mu mom) + d^): product and sum on |mom mu|, the sum on |d|:               |err| <= bd + 2 u |mom mu| + u |d|      =: bmu
  p'     fl(p - fl(mu' lr)): the product, the difference rounds |p| + |lr mu'| once:     |err| <= lr bmu + u |p| + 2 u |lr mu'|
Bounds are evaluated from the inputs and the float64 reference only.
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16
RSQRT_ULP = 2
BN_MAX_BLOCKS, BN_MIN_TRIPS = 1024, 4
SP_LANES = 32
LARS_BLOCKS = 1024
LARS_WRAP = LARS_BLOCKS * 256 * 4   # elements one grid pass of lars_sumsq_kernel covers
F = np.float32


def f32(x) -> float:
    return float(F(x))


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _d(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ geometry
def bn_geometry(rows: int, dim: int) -> dict:
    assert dim % 4 == 0 and 4 <= dim <= 1024 and rows >= 1
    d4 = dim // 4
    rp = 256 // d4
    want = min(cdiv(rows, rp * BN_MIN_TRIPS), BN_MAX_BLOCKS)
    slice_rows = cdiv(cdiv(rows, want), rp) * rp
    grid = cdiv(rows, slice_rows)
    trips = slice_rows // rp
    return dict(d4=d4, rp=rp, slice=slice_rows, grid=grid, trips=trips, tail=trips + rp + cdiv(grid, SP_LANES) + SP_LANES,
                scratch_bytes=(grid + 3) * dim * 4)


def sumsq_chain(n: int) -> int:
    n4 = n // 4
    grid = max(1, min(cdiv(n4, 256), LARS_BLOCKS))
    return cdiv(n4, grid * 256) + cdiv(grid, 256) + 22


# ------------------------------------------------------------------------------------------------ the operations, fp64
def bn_train(x, running_mean=None, running_var=None, eps=1e-6, momentum=0.1) -> dict:
    """dict(y, mean, var, rstd, unbiased, running_mean, running_var (None when not tracked), asum = sum_r |x - x[0]|)."""
    x = _d(x)
    rows = x.shape[0]
    assert rows >= 2
    eps, mom = f32(eps), f32(momentum)
    mean = x.sum(0) / rows
    d = x - mean
    var = (d * d).sum(0) / rows
    rstd = 1.0 / np.sqrt(var + eps)
    unb = var * rows / (rows - 1)
    rm = rv = None
    if running_mean is not None:
        rm = (1.0 - mom) * _d(running_mean) + mom * mean
        rv = (1.0 - mom) * _d(running_var) + mom * unb
    return dict(y=d * rstd, mean=mean, var=var, rstd=rstd, unbiased=unb, running_mean=rm, running_var=rv, d=d, asum=np.abs(x - x[0]).sum(0))


def bn_eval(x, running_mean, running_var, eps=1e-6) -> dict:
    d = _d(x) - _d(running_mean)
    rstd = 1.0 / np.sqrt(_d(running_var) + f32(eps))
    return dict(y=d * rstd, mean=_d(running_mean), rstd=rstd, d=d)


def bn_train_bounds(ref: dict, rows: int, dim: int, running_mean=None, running_var=None, eps=1e-6, momentum=0.1) -> dict:
    """dict(mean, var, rstd, y, running_mean, running_var) of bounds; the counts are in the module docstring."""
    tail = bn_geometry(rows, dim)["tail"]
    eps, mom = f32(eps), f32(momentum)
    k0, k2 = 1 + tail, 3 + tail
    bm = SECOND * ((k0 + 2) * U * ref["asum"] / rows + U * np.abs(ref["mean"]))
    bv = SECOND * ((k2 + 2) * U * (ref["var"] + bm * bm) + bm * bm)
    t = bv / (ref["var"] + eps) + U
    rel = SECOND * (0.5 * t * (1.0 + t) + RSQRT_ULP * 2.0 * U)
    a = ref["d"] * ref["rstd"]
    by = SECOND * (ref["rstd"] * bm + np.abs(a) * (rel + 2.0 * U))
    out = dict(mean=bm, var=bv, rstd=ref["rstd"] * rel, y=by, running_mean=None, running_var=None)
    if running_mean is not None:
        keep = 1.0 - mom
        bm2 = rows * (k2 * U * (ref["var"] + bm * bm) + bm * bm)
        out["running_mean"] = SECOND * (3.0 * U * np.abs(keep * _d(running_mean)) + 2.0 * U * np.abs(mom * ref["mean"]) + mom * bm)
        out["running_var"] = SECOND * (3.0 * U * np.abs(keep * _d(running_var)) + 2.0 * U * mom * ref["unbiased"]
                                       + mom * (bm2 / (rows - 1) + 2.0 * U * ref["unbiased"]))
    return out


def bn_eval_bounds(ref: dict) -> dict:
    rel = SECOND * (0.5 * U * (1.0 + U) + RSQRT_ULP * 2.0 * U)
    return dict(rstd=ref["rstd"] * rel, y=SECOND * np.abs(ref["d"] * ref["rstd"]) * (rel + 2.0 * U))


def lars_step(p, g, mu, adapt, lr, momentum, weight_decay, trust_coefficient) -> dict:
    """dict(p, mu, pn, un, q, and the terms the bounds need).  adapt = 0: pn = |p|, un = |g| (what norms_out reports), q = 1."""
    p, g, mu = _d(p), _d(g), _d(mu)
    lr, mom, wd, tc = f32(lr), f32(momentum), f32(weight_decay) if adapt else 0.0, f32(trust_coefficient)
    dp = g + wd * p
    pn, un = math.sqrt(float(np.dot(p, p))), math.sqrt(float(np.dot(dp, dp)))
    q = tc * pn / un if (adapt and pn > 0.0 and un > 0.0) else 1.0
    d = dp * q
    mu2 = mom * mu + d
    return dict(p=p - lr * mu2, mu=mu2, pn=pn, un=un, q=q, d=d, dp=dp, e=2.0 * U * (np.abs(g) + np.abs(wd * p)) if adapt else np.zeros_like(p),
                mom_mu=mom * mu, p0=p, lr=lr, adapt=bool(adapt))


def lars_bounds(ref: dict, n: int) -> dict:
    """dict(p, mu, pn, un) of bounds for a step over n elements."""
    k = sumsq_chain(n)
    rel_pn = (k / 2 + 1) * U
    e2 = math.sqrt(float(np.dot(ref["e"], ref["e"])))
    bun = SECOND * (e2 + (k / 2 + 1) * U * (ref["un"] + e2))
    if ref["adapt"] and ref["pn"] > 0.0 and ref["un"] > 0.0:
        r = bun / ref["un"]
        rel_q = SECOND * (rel_pn + 2.0 * U + r) / (1.0 - r) if r < 1.0 else math.inf
        bd = ref["q"] * (1.0 + rel_q) * ref["e"] + np.abs(ref["d"]) * (rel_q + U)
    elif ref["adapt"]:
        bd = ref["e"] + U * np.abs(ref["d"])   # q = 1 exactly: dp^ alone
    else:
        bd = np.zeros_like(ref["d"])
    bmu = SECOND * (bd + 2.0 * U * np.abs(ref["mom_mu"]) + U * np.abs(ref["d"]))
    bp = SECOND * (ref["lr"] * bmu + U * np.abs(ref["p0"]) + 2.0 * U * np.abs(ref["lr"] * ref["mu"]))
    return dict(p=bp, mu=bmu, pn=SECOND * rel_pn * ref["pn"], un=bun)


def fold(weight, bias, running_mean, running_var, eps=1e-6):
    """(W', b'): W'[c][d] = W[c][d] / sqrt(var[d] + eps), b'[c] = b[c] - sum_d W'[c][d] mean[d]."""
    wf = _d(weight) / np.sqrt(_d(running_var) + f32(eps))[None, :]
    return wf, _d(bias) - wf @ _d(running_mean)


def head(y, weight, bias, labels=None) -> dict:
    """Logits of the linear layer and, with labels, the mean cross-entropy, the correct count, dW and db."""
    y, w, b = _d(y), _d(weight), _d(bias)
    logits = y @ w.T + b
    out = dict(logits=logits)
    if labels is not None:
        lab = np.asarray(labels, dtype=np.int64)
        z = logits - logits.max(1, keepdims=True)
        lse = np.log(np.exp(z).sum(1, keepdims=True))
        logp = z - lse
        n = y.shape[0]
        dl = np.exp(logp)
        dl[np.arange(n), lab] -= 1.0
        dl /= n
        out.update(loss=float(-logp[np.arange(n), lab].mean()), correct=int((logits.argmax(1) == lab).sum()), dW=dl.T @ y, db=dl.sum(0))
    return out


def linear_bound(x, weight, bias, x_bound=None):
    """Bound of fp32 logits x W^T + b against float64, for fp32 W and b given exactly: a dot product of D products summed in any order
    is off by at most (D + 1) u sum_d |x_d W_cd| with the bias addition ((D - 1) additions, the product, the bias), and the bias itself
    enters unrounded.  x_bound (per element, optional): the error x already carries, which the layer passes on as sum_d |W_cd| x_bound_d."""
    x, w, b = np.abs(_d(x)), np.abs(_d(weight)), np.abs(_d(bias))
    out = SECOND * (x.shape[1] + 1) * U * (x @ w.T + b)
    if x_bound is not None:
        out = out + SECOND * (_d(x_bound) @ w.T)
    return out


def probe_step(weight, bias, mu_w, mu_b, running_mean, running_var, feats, labels, lr, cfg) -> dict:
    """One LinearProbe.step in float64: dict(bn, head, lars_w, lars_b) of the pieces above."""
    bn = bn_train(feats, running_mean, running_var, cfg["bn_eps"], cfg["bn_momentum"])
    h = head(bn["y"], weight, bias, labels)
    lw = lars_step(_d(weight).reshape(-1), h["dW"].reshape(-1), mu_w, 1, lr, cfg["momentum"], cfg["weight_decay"], cfg["trust_coefficient"])
    lb = lars_step(bias, h["db"], mu_b, 0, lr, cfg["momentum"], cfg["weight_decay"], cfg["trust_coefficient"])
    return dict(bn=bn, head=h, lars_w=lw, lars_b=lb)


# ------------------------------------------------------------------------------------------------ data
BN_SHAPES = [(2, 4), (3, 144), (257, 148), (1031, 384), (4096, 1024)]
CONST_VALUE = f32(2.7182817)


def const_column(dim: int) -> int:
    return dim // 2 + 1


def gen_bn(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    """(rows, dim) fp32: column means spread over +-8, standard deviations over [0.05, 4] (log-spaced, both shuffled), one exactly constant
    column (const_column) -- what LayerNorm outputs look like to a one-sweep variance: means far from zero beside small spreads."""
    r = np.random.default_rng([rows, dim, seed])
    means = r.permutation(np.linspace(-8.0, 8.0, dim))
    stds = r.permutation(np.geomspace(0.05, 4.0, dim))
    x = (means + stds * r.standard_normal((rows, dim))).astype(F)
    x[:, const_column(dim)] = CONST_VALUE
    return x


def gen_bn_exact(rows: int, dim: int, seed: int = 0) -> np.ndarray:
    """Small integers: every difference from the pivot row and every partial sum is exact, and at a power-of-two row count so is the mean."""
    return np.random.default_rng([rows, dim, seed, 7]).integers(-8, 9, (rows, dim)).astype(F)


def gen_running(dim: int, seed: int = 0):
    r = np.random.default_rng([dim, seed, 11])
    return r.standard_normal(dim).astype(F), (0.5 + r.random(dim)).astype(F)


def one_sweep_var_fp32(x: np.ndarray) -> np.ndarray:
    """The variance a one-sweep fp32 kernel would form: E[x^2] - E[x]^2 with fp32 accumulators (numpy's pairwise sums, kinder than a kernel's)."""
    x = np.asarray(x, dtype=F)
    n = F(x.shape[0])
    m = x.sum(0, dtype=F) / n
    return (x * x).sum(0, dtype=F) / n - m * m


def gen_lars(n: int, seed: int = 0, zero_p: bool = False, zero_g: bool = False, zero_mu: bool = False):
    """(p, g, mu) fp32: weights of a probe head's size, gradients three decades smaller, a momentum buffer of the gradients' size."""
    r = np.random.default_rng([n, seed, 13])
    p = (0.01 * r.standard_normal(n)).astype(F)
    g = (1e-3 * r.standard_normal(n) * 10.0 ** r.uniform(-2.0, 0.0, n)).astype(F)
    mu = (1e-3 * r.standard_normal(n)).astype(F)
    if zero_p:
        p[:] = 0.0
    if zero_g:
        g[:] = 0.0
    if zero_mu:
        mu[:] = 0.0
    return p, g, mu


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
