"""float64 restatement of the optimizer step (k_loss_optim.hip) for the tests, and per-element error bounds of the fp32 kernels.

numpy on the CPU, float64 throughout.  Hyperparameters enter as the fp32 values the C ABI receives, widened to double (``f32``).

  adamw   torch.optim.AdamW, single group (oracle/mae_oracle.py:adamw_step): decoupled decay, then
          denom = sqrt(v') / sqrt(1 - b2^step) + eps, then p' -= lr / (1 - b1^step) * m' / denom; the gradient is first
          multiplied by the clip coefficient.
  sumsq / clip   torch.nn.utils.clip_grad_norm_: norm = sqrt(sum g^2), coef = min(1, max_norm / (norm + 1e-6)).
  ema     t' = mom * t + (1 - mom) * p_new (the I-JEPA target encoder).
  bf16_rne       round-to-nearest-even of fp32 to bf16 as bit arithmetic: the operand copies the GEMMs read.
  wcache_layout  where mae_engine_create puts the transposed bf16 copy of every GEMM weight.

Bounds.  u = 2^-24 is the fp32 unit roundoff: every fp32 operation returns x (1 + d) with |d| <= u, division and square root
included (hipcc rounds both correctly by default).  A value that went through k such operations is x (1 + t_k) with
|t_k| <= k u to first order; every chain here has k <= 64, so the second-order terms stay below k u <= 2^-18 of the
first-order bound and the factor SECOND = 1 + 2^-16 covers them.  Fused multiply-adds (the library is built with
-ffp-contract=fast) only remove roundings from a chain, so the counts hold whichever products the compiler fuses.  All counts
need normal numbers: the data generator keeps every intermediate away from the denormals.

adamw_kernel, with c = stats[1], A = |b1 m| + |(1 - b1) g c|, and 1 - b1, 1 - b2 exact (Sterbenz: b in [0.5, 1]):
  m' = fl(fl(m b1) + fl(fl(g c) (1 - b1)))
       m-term: product, sum = 2; g-term: g c, product, sum = 3                              |m' err| <= 3 u A
  v' = fl(fl(v b2) + fl(fl(fl(g c)^2) (1 - b2)))
       v-term: product, sum = 2; g-term: g c twice (it is squared), square, product, sum = 5; both terms are positive
                                                                                           |v' err| <= 5 u v'
  p' = fl(fl(p decay) - fl(step q)),   decay = fl(1 - fl(lr wd)),  step = fl(lr fl(1 / bc1)),  q = fl(m' / denom)
       decay: fl(lr wd) moves it by u lr wd, the subtraction by u / 2 (the result lies in [0.5, 1]), together <= u decay for
       lr wd <= 1/4 = 1; product = 1; the final subtraction rounds |p decay| + |step q| once = 1     -> 3 on |p decay|
       denom = fl(fl(sqrt(v')) inv + eps), inv = fl(1 / fl(sqrt(fl(bc2)))):
               sqrt(v') = 5/2 + 1; inv = 1/2 + 1 + 1 = 5/2, product = 1; the sum with eps (exact, positive) = 1 -> 8
       q:      m' is off by 3 u A and |m'| <= A; denom = 8; the division = 1                      -> 3 + 8 + 1 = 12 on A / denom
       step:   fl(bc1), the reciprocal, the product = 3; fl(step q) = 1; the final subtraction = 1 -> 12 + 5 = 17
                                                     |p' err| <= u (3 |p decay| + 17 step A / denom)
  EMA  t' = fl(fl(t mom) + fl(p' fl(1 - mom))): t-term 2, p-term 3       |t' err| <= 3 u (|mom t| + |(1 - mom) p'|)

sumsq_kernel -> block_sum_256 -> finalize, all summands positive, so the relative error is at most the longest chain of
roundings one summand goes through:
  the square 1, the three additions inside v0^2 + v1^2 + v2^2 + v3^2 3, one `acc +=` per grid-stride pass I,
  wave_sum 6 (shuffles of 32 .. 1), red[0] + red[1] + red[2] + red[3] 3, the finalize kernel's strided loop F = ceil(grid / 256),
  its wave_sum 6 and its four-way sum 3:               k = I + F + 22,  I = ceil((n / 4) / (grid 256)), grid = min(ceil(n / 1024), 1024)
  accumulate = 1 adds the prior total once more:       |err| <= k u s + u (prior + s)
  norm = fl(sqrt(sumsq)):                              (k / 2 + 1) u relative
  coef = min(1, fl(max_norm / fl(norm + 1e-6f))):      (k / 2 + 3) u relative, of the unclamped quotient
"""
from __future__ import annotations

import math

import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16
CLIP_EPS = float(np.float32(1e-6))   # the kernels add 1e-6f
TRAINABLE, MATRIX = 1, 8              # MAE_PARAM_TRAINABLE, MAE_PARAM_MATRIX
RED_BLOCKS, ADAMW_BLOCKS = 1024, 256 * 16
SUMSQ_WRAP = RED_BLOCKS * 256 * 4     # elements one pass of sumsq_kernel covers
ADAMW_WRAP = ADAMW_BLOCKS * 256 * 4   # elements one pass of adamw_kernel covers

B1, B2, EPS = 0.9, 0.999, 1e-8
# the hyperparameter sets of the tests: coef None = the clip coefficient of the generated gradient for max_norm = 0.37 * its norm
HYPER = {
    "step1": dict(step=1, lr=1e-3, wd=0.05, coef=None),
    "step2": dict(step=2, lr=1e-3, wd=0.05, coef=0.37),
    "late": dict(step=100000, lr=1e-3, wd=0.0, coef=None),
    "warmup": dict(step=1, lr=5.9e-5, wd=0.05, coef=None),   # the production warm-up learning rate
}


def f32(x) -> float:
    """A Python float as the C ABI passes it: rounded to fp32, widened to double."""
    return float(np.float32(x))


def _d(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


# ------------------------------------------------------------------------------------------------ the operations, fp64
def adamw_terms(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    """Everything the bounds need, in float64: dict(p, m, v, pd = p decay, A, upd = lr / bc1 * A / denom)."""
    p, g, m, v = _d(p), _d(g), _d(m), _d(v)
    coef, lr, b1, b2, eps, wd = float(coef), f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
    bc1, bc2 = 1.0 - b1 ** int(step), 1.0 - b2 ** int(step)
    gc = g * coef
    pd = p * (1.0 - lr * wd)
    a_m, a_g = b1 * m, (1.0 - b1) * gc
    m2 = a_m + a_g
    v2 = b2 * v + (1.0 - b2) * gc * gc
    denom = np.sqrt(v2) / math.sqrt(bc2) + eps
    k = (lr / bc1) / denom
    return dict(p=pd - k * m2, m=m2, v=v2, pd=pd, A=np.abs(a_m) + np.abs(a_g), upd=k * (np.abs(a_m) + np.abs(a_g)))


def adamw(p, g, m, v, coef, lr, b1, b2, eps, wd, step):
    """(p', m', v') of one AdamW step on g * coef."""
    t = adamw_terms(p, g, m, v, coef, lr, b1, b2, eps, wd, step)
    return t["p"], t["m"], t["v"]


def adamw_bounds(t, b1=B1, b2=B2, lr=1e-3, wd=0.05):
    """(bound p', bound m', bound v') from adamw_terms; the counts are in the module docstring."""
    assert 0.5 <= f32(b1) <= 1.0 and 0.5 <= f32(b2) <= 1.0 and f32(lr) * f32(wd) <= 0.25, "the counts assume these ranges"
    return (SECOND * U * (3.0 * np.abs(t["pd"]) + 17.0 * t["upd"]), SECOND * 3.0 * U * t["A"], SECOND * 5.0 * U * t["v"])


def sumsq(g) -> float:
    g = _d(g)
    return float(np.dot(g, g))


def clip(total_sumsq: float, max_norm) -> tuple:
    """(norm, coef) as clip_grad_norm_ computes them."""
    norm = math.sqrt(float(total_sumsq))
    return norm, min(1.0, f32(max_norm) / (norm + CLIP_EPS))


def ema(t, p_new, mom):
    mom = f32(mom)
    return mom * _d(t) + (1.0 - mom) * _d(p_new)


def ema_bound(t, p_new, mom):
    mom = f32(mom)
    return SECOND * 3.0 * U * (np.abs(mom * _d(t)) + np.abs((1.0 - mom) * _d(p_new)))


def sumsq_chain(n: int) -> int:
    """k of the module docstring for a sum of squares over n elements."""
    n4 = n // 4
    grid = max(1, min(-(-n4 // 256), RED_BLOCKS))
    passes = -(-n4 // (grid * 256))
    return passes + -(-grid // 256) + 22


def sumsq_rel_bound(n: int) -> float:
    return SECOND * sumsq_chain(n) * U


def norm_rel_bound(k: int) -> float:
    return SECOND * (k / 2 + 1) * U


def coef_rel_bound(k: int) -> float:
    return SECOND * (k / 2 + 3) * U


# ------------------------------------------------------------------------------------------------ bf16
def bf16_rne(x) -> np.ndarray:
    """The bf16 bit patterns (uint16) of fp32 values rounded to nearest, ties to even: add 0x7FFF plus the lowest kept bit to
    the fp32 pattern, keep the upper half.  A NaN keeps its upper half with the quiet bit set."""
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32, x.dtype
    bits = x.view(np.uint32).astype(np.uint64)
    hi = bits >> np.uint64(16)
    rounded = (bits + np.uint64(0x7FFF) + (hi & np.uint64(1))) >> np.uint64(16)
    nan = (bits & np.uint64(0x7FFFFFFF)) > np.uint64(0x7F800000)
    return np.where(nan, hi | np.uint64(0x40), rounded).astype(np.uint16)


def bf16_truncate(x) -> np.ndarray:
    """The upper half of the fp32 pattern: what a copy that forgets to round would write."""
    return (np.ascontiguousarray(x).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the weight cache
def _round_up(a: int, b: int) -> int:
    return -(-a // b) * b


def wcache_layout(table, trainable_elems: int):
    """(matrices, trans_elems): for every MAE_PARAM_MATRIX | TRAINABLE entry of ``Engine.table`` (name, offset, numel, shape,
    flags), in table order, dict(name, offset, numel, rows, cols, t_off, t_abs).  t_off is the running sum of round_up(numel, 64)
    as in mae_engine_create; the transposed copy (cols x rows) starts t_abs = trainable_elems + t_off bf16 elements into wcache."""
    out, toff = [], 0
    for name, offset, numel, shape, flags in table:
        if flags & TRAINABLE and flags & MATRIX:
            rows = int(shape[0])
            out.append(dict(name=name, offset=int(offset), numel=int(numel), rows=rows, cols=int(numel) // rows, t_off=toff,
                            t_abs=int(trainable_elems) + toff))
            toff += _round_up(int(numel), 64)
    return out, toff


def transposed_ref(p32: np.ndarray, mat) -> np.ndarray:
    """The bf16 bits of matrix ``mat``'s transposed copy, flat, from the fp32 arena."""
    w = p32[mat["offset"]:mat["offset"] + mat["numel"]].reshape(mat["rows"], mat["cols"])
    return bf16_rne(np.ascontiguousarray(w.T)).reshape(-1)


# ------------------------------------------------------------------------------------------------ data
def gen_grad(n: int, seed: int) -> np.ndarray:
    """sign * 10^U(-12, 2) with exact zeros (one element in 64): fourteen decades, (1 - b2) g^2 stays a normal fp32 number."""
    r = np.random.default_rng([seed, 1])
    g = np.where(r.random(n) < 0.5, -1.0, 1.0) * 10.0 ** r.uniform(-12.0, 2.0, n)
    g[r.random(n) < 1 / 64] = 0.0
    return g.astype(np.float32)


def gen_params(n: int, seed: int) -> np.ndarray:
    """normal * 10^U(-4, 1) with exact (+0) zeros."""
    r = np.random.default_rng([seed, 2])
    p = r.standard_normal(n) * 10.0 ** r.uniform(-4.0, 1.0, n)
    p[r.random(n) < 1 / 64] = 0.0
    return p.astype(np.float32)


def gen_state(g: np.ndarray, step: int, coef: float, seed: int, b1=B1):
    """(m, v) before step ``step``: zeros at step 1; later v = 10^U(-2, 2) g^2, m = normal * 10^U(-1, 1) * |g| (normal * 1e-3
    where g is zero), and one stripe (64 elements in every 1024) with m = -(1 - b1) / b1 * g * coef, so that m' cancels to
    rounding noise while the bound keeps the size of its two terms."""
    n = g.size
    if step == 1:
        return np.zeros(n, np.float32), np.zeros(n, np.float32)
    r = np.random.default_rng([seed, 3])
    gd = g.astype(np.float64)
    v = (10.0 ** r.uniform(-2.0, 2.0, n) * gd * gd).astype(np.float32)
    m = r.standard_normal(n) * 10.0 ** r.uniform(-1.0, 1.0, n) * np.where(gd == 0.0, 1e-3, np.abs(gd))
    stripe = (np.arange(n) % 1024 >= 256) & (np.arange(n) % 1024 < 320)
    b1 = f32(b1)
    m[stripe] = -(1.0 - b1) / b1 * gd[stripe] * float(coef)
    return m.astype(np.float32), v


def gen_case(n: int, hyper: str, seed: int):
    """dict(p, g, m, v fp32 arrays of n elements, coef as the fp32 value in stats[1], norm, and the hyperparameters)."""
    h = HYPER[hyper]
    g = gen_grad(n, seed)
    norm = math.sqrt(sumsq(g))
    coef = h["coef"] if h["coef"] is not None else clip(norm * norm, 0.37 * norm)[1]
    coef = f32(coef)
    m, v = gen_state(g, h["step"], coef, seed)
    return dict(p=gen_params(n, seed), g=g, m=m, v=v, coef=coef, norm=norm, step=h["step"], lr=h["lr"], wd=h["wd"], b1=B1, b2=B2, eps=EPS)


def hyper_args(c):
    return dict(lr=c["lr"], b1=c["b1"], b2=c["b2"], eps=c["eps"], wd=c["wd"], step=c["step"])


# ------------------------------------------------------------------------------------------------ comparison
def worst_ratio(out, ref, bound) -> float:
    """max |out - ref| / bound; an error where the bound is zero (exact zeros in, exact zeros out) counts as infinite."""
    err = np.abs(_d(out) - ref)
    if not np.all(np.isfinite(err)):
        return math.inf
    zero = bound == 0.0
    if np.any(err[zero] != 0.0):
        return math.inf
    return float(np.max(err[~zero] / bound[~zero])) if np.any(~zero) else 0.0


def adamw_ratios(p_out, m_out, v_out, c, coef=None):
    """Worst error / bound of (p', m', v') for case ``c`` (gen_case) against the fp64 AdamW; coef defaults to the case's."""
    t = adamw_terms(c["p"], c["g"], c["m"], c["v"], c["coef"] if coef is None else coef, **hyper_args(c))
    bp, bm, bv = adamw_bounds(t, c["b1"], c["b2"], c["lr"], c["wd"])
    return dict(p=worst_ratio(p_out, t["p"], bp), m=worst_ratio(m_out, t["m"], bm), v=worst_ratio(v_out, t["v"], bv))
