"""float64 numpy restatement of the t-SNE kernels (k_tsne.hip) and of embedding.DeviceTSNE, the per-element error bounds of the fp32
kernels against it, and the blob data of the end-to-end tests.  numpy only: tests/test_tsne_ref_host.py pins it to sklearn's internals.

Reference
  sqdist(x)                    d_ij = sum_k (x_ik - x_jk)^2
  search(D, perplexity)        sklearn's _binary_search_perplexity per row on D less the row's minimum over j != i (P is unchanged by
                               the shift): beta from 1, doubled / halved until bracketed, then bisected, <= 100 steps, tol 1e-5
                               -> p_cond, beta, steps, H.  The row keeps the p of the last beta it evaluated, as sklearn's does.
  entropy(D, beta) / softmax(D, beta)   H_i and p_j|i at a given beta
  joint(p_cond)                (p_j|i + p_i|j) / (2 n)
  gradient(P, y, alpha)        grad = 4 (alpha a - r / Z), KL = sum_{i != j} p (log p - log w) + log Z, and the absolute sums the bounds need
  update(...)                  sklearn's _gradient_descent step, in the dtype of its inputs: with float32 arrays and float32 scalars every
                               numpy operation rounds once, which is what the kernel does (no contraction) -- bit for bit
  fit(x, init, ...)            the whole DeviceTSNE.fit in float64

Bounds, first order, counted from the kernel's statements.  u = 2^-24; E_EXP = E_RCP = E_LOG = 2 u: one ulp of v_exp_f32, v_rcp_f32 and
logf as the ISA manual and the ocml state them (taken from there, as tests/gemm_ref.py does, not measured); SECOND = 1 + 2^-6 covers
products of first-order terms; TINY = 2^-120 covers results flushed below the normal range.
  sqdist  the difference rounds once (2 u on its square), dim fused multiply-adds each round a partial sum <= d:   (dim + 2) u d
  p_cond  (against the float64 softmax of the DEVICE's distances at the DEVICE's beta: the inputs are then exact.)  X_j = beta d'_j:
          d' = d - m rounds (u X), beta d' rounds (u X), __expf multiplies by a rounded log2 e and rounds the product (2 u X), v_exp_f32
          E_EXP:  eE_j = 4 u X_j + E_EXP.  S: a thread adds ceil(n / 256) terms in order, 6 butterfly levels, 3 wave sums, all terms
          >= 0:  eS = sum_j p_j eE_j + (ceil(n / 256) + 8) u.  One correctly rounded division:   |dp_j| <= p_j (eE_j + eS + u)
  H       T = sum d'_j e_j: terms carry eE_j + u, the same depth.  beta T / S: one division, one product.  logf(S): eS + E_LOG |log S|.
          The sum, the subtraction of fl(log perplexity) and its rounding: 2 u (|H| + |log perplexity|):
          slack_i = eS + E_LOG |log S| + B (eT + eS + 3 u) + 2 u (|H| + |log perp|),  B = beta E_p[d'], eT = sum_j t_j (eE_j + u) / T + depth u
  P       fl(fl(p_j|i + p_i|j) / fl(2 n)) from the device's own p_cond is exact arithmetic in fp32: compared bit for bit.
  grad    dx = fl(y_i - y_j): u.  q = fma(dx, dx, fma(dy, dy, 1)): 2 u from each square's operand, two roundings <= u q: 4 u.
          w = v_rcp(q): 6 u.  p w: 7 u; the a-term (p w) dx: 8 u.  w^2: 13 u; the r-term: 14 u.  A lane adds 4 ceil(pitch / 256)
          terms in order, then 6 butterfly levels: La = 4 ceil(pitch / 256) + 6 roundings, each <= u sum |terms|.
            ba_i = (8 + La) u sum_j |p w dx|,  br_i = (14 + La) u sum_j w^2 |dx|,  z_i relative (6 + La) u
          Z adds n row sums at depth Lz = ceil(n / 256) + 8:  eZ = (6 + La + Lz) u.  r / Z rounds once, the fma once, 4 x is exact:
            bg = 4 (alpha ba + (br + |r| (eZ + u)) / Z + u |alpha a - r / Z|)
  KL      a term p (logf p + logf q): E_LOG on each logarithm, 4 u absolute from q, one rounding of the sum:  p u (3 |log p| + 3 log q + 4);
          accumulation (La + Lz) u sum p (|log p| + log q);  log Z: eZ + E_LOG |log Z|;  the last sum u |KL|.
  step    gains is exact wherever the sign of update * grad cannot flip: |grad| > bg (update is an exact input).  update' =
          fl(fl(mom u) - fl(lr fl(g gains))), gains off its float64 value by u (0.2f, 0.8f and one rounding):
          lr gains bg + u (|mom u| + 3 lr |g| gains + |update'|);  y' adds u |y'|.  Where the sign may flip, the two candidate gains
          differ by dG and the step by lr (|g| + bg) dG more.
"""
from __future__ import annotations

import math

import numpy as np

U32 = 2.0 ** -24
E_EXP = E_RCP = E_LOG = 2 * U32
SECOND = 1.0 + 2.0 ** -6
TINY = 2.0 ** -120
MAX_STEPS, TOL = 100, 1e-5
F = np.float32


def pitch_of(n: int) -> int:
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------------------------------------ data
def blobs(clusters: int = 6, per: int = 100, dim: int = 32, seed: int = 0):
    """(x (n, dim) fp32, labels (n,)): Gaussian clusters, centres of standard deviation 6 / sqrt 2, unit noise, rows shuffled."""
    r = np.random.default_rng(seed)
    centres = r.standard_normal((clusters, dim)) * (6.0 / math.sqrt(2.0))
    labels = np.repeat(np.arange(clusters), per)
    x = centres[labels] + r.standard_normal((clusters * per, dim))
    perm = r.permutation(clusters * per)
    return x[perm].astype(F), labels[perm]


def gen_features(n: int, dim: int, seed: int = 0, case: str = "plain") -> np.ndarray:
    """(n, dim) fp32 rows in three loose clusters; case "twins": rows 1 and n - 2 identical; "outlier": row 2 far from everything."""
    r = np.random.default_rng([n, dim, seed, 5])
    x = r.standard_normal((n, dim)) + 2.0 * r.standard_normal((3, dim))[r.integers(0, 3, n)]
    if case == "twins":
        x[n - 2] = x[1]
    elif case == "outlier":
        x[2] += 300.0
    elif case != "plain":
        raise ValueError(case)
    return x.astype(F)


def loo_1nn_accuracy(Z, labels) -> float:
    Z = np.asarray(Z, dtype=np.float64)
    D = sqdist(Z)
    np.fill_diagonal(D, np.inf)
    return float(np.mean(labels[D.argmin(1)] == labels))


# ------------------------------------------------------------------------------------------------ affinities
def sqdist(x) -> np.ndarray:
    x = np.asarray(x, dtype=np.float64)
    out = np.empty((x.shape[0], x.shape[0]))
    for i in range(x.shape[0]):   # the difference form: no cancellation between large norms
        out[i] = ((x[i] - x) ** 2).sum(1)
    return out


def sqdist_bound(D64, dim: int) -> np.ndarray:
    return SECOND * (dim + 2) * U32 * D64 + TINY


def _shifted(D, i):
    d = np.asarray(D[i], dtype=np.float64)
    m = np.delete(d, i).min()
    d = d - m
    d[i] = 0.0   # never used: every sum skips j = i
    return d


def _row_stats(dsh, i, beta):
    """e_j (0 at i), S, T of row i at beta on shifted distances."""
    e = np.exp(-beta * dsh)
    e[i] = 0.0
    return e, e.sum(), (dsh * e).sum()


def entropy(D, beta) -> np.ndarray:
    out = np.empty(len(beta))
    for i in range(len(beta)):
        _, S, T = _row_stats(_shifted(D, i), i, float(beta[i]))
        out[i] = math.log(S) + float(beta[i]) * T / S
    return out


def softmax(D, beta) -> np.ndarray:
    out = np.empty((len(beta), len(beta)))
    for i in range(len(beta)):
        e, S, _ = _row_stats(_shifted(D, i), i, float(beta[i]))
        out[i] = e / S
    return out


def search(D, perplexity: float, beta_dtype=np.float64):
    """-> dict(p_cond (n, n), beta (n), steps (n), H (n)).  steps = evaluations of H (100 = not converged).  beta_dtype float32
    restates the kernel's beta arithmetic (the sums stay float64)."""
    n = D.shape[0]
    desired = math.log(perplexity)
    p_cond, betas, steps, Hs = np.zeros((n, n)), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n)
    T_ = beta_dtype
    for i in range(n):
        dsh = _shifted(D, i)
        beta, lo, hi = T_(1.0), -np.inf, np.inf
        for step in range(MAX_STEPS):
            e, S, T = _row_stats(dsh, i, float(beta))
            H = math.log(S) + float(beta) * T / S
            diff = H - desired
            if abs(diff) <= TOL or step == MAX_STEPS - 1:
                break
            if diff > 0.0:
                lo = beta
                beta = T_(beta * T_(2.0)) if hi == np.inf else T_((beta + hi) / T_(2.0))
            else:
                hi = beta
                beta = T_(beta / T_(2.0)) if lo == -np.inf else T_((beta + lo) / T_(2.0))
        p_cond[i], betas[i], steps[i], Hs[i] = e / S, float(beta), step + 1, H
    return dict(p_cond=p_cond, beta=betas, steps=steps, H=Hs)


def joint(p_cond) -> np.ndarray:
    return (p_cond + p_cond.T) / (2.0 * p_cond.shape[0])


def affinities(x, perplexity: float) -> np.ndarray:
    return joint(search(sqdist(x), perplexity)["p_cond"])


def search_bounds(D, beta, perplexity: float):
    """-> (p_bound (n, n), H_slack (n)) for the device's distances D (fp32 values) and the device's beta."""
    n = len(beta)
    depth = math.ceil(n / 256) + 8
    pb, slack = np.empty((n, n)), np.empty(n)
    for i in range(n):
        dsh, b = _shifted(D, i), float(beta[i])
        e, S, T = _row_stats(dsh, i, b)
        p = e / S
        eE = 4 * U32 * b * dsh + E_EXP
        eE[i] = 0.0
        eS = float((p * eE).sum()) + depth * U32
        pb[i] = SECOND * p * (eE + eS + U32) + TINY
        pb[i, i] = 0.0
        t = dsh * e
        eT = (float((t * (eE + U32)).sum()) / T if T > 0 else 0.0) + depth * U32
        B = b * T / S
        H = math.log(S) + B
        slack[i] = SECOND * (eS + E_LOG * abs(math.log(S)) + B * (eT + eS + 3 * U32) + 2 * U32 * (abs(H) + abs(math.log(perplexity))))
    return pb, slack


# ------------------------------------------------------------------------------------------------ gradient
def gradient(P, y, alpha: float) -> dict:
    """P (n, n) (any padding cut off), y (n, 2) -> dict(grad, kl, a, r, Z, and the absolute sums of the bounds), all float64."""
    P, y = np.asarray(P, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    diff = y[:, None, :] - y[None, :, :]                 # (n, n, 2): y_i - y_j
    q = 1.0 + (diff ** 2).sum(-1)
    w = 1.0 / q
    off = ~np.eye(n, dtype=bool)
    a = ((P * w)[:, :, None] * diff).sum(1)
    r = ((w * w)[:, :, None] * diff).sum(1)
    Z = float((w * off).sum())
    pos = off & (P > 0)
    logp = np.zeros_like(P)
    logp[pos] = np.log(P[pos])
    logq = np.log(q)
    kl_terms = np.where(pos, P * (logp + logq), 0.0)
    kl = float(kl_terms.sum()) + math.log(Z)
    return dict(grad=4.0 * (alpha * a - r / Z), kl=kl, a=a, r=r, Z=Z,
                abs_a=((P * w)[:, :, None] * np.abs(diff)).sum(1), abs_r=((w * w)[:, :, None] * np.abs(diff)).sum(1),
                kl_abs=float(np.where(pos, P * (np.abs(logp) + logq), 0.0).sum()), kl_p=float(np.where(pos, P, 0.0).sum()))


def gradient_depths(n: int):
    La = 4 * math.ceil(pitch_of(n) / 256) + 6
    Lz = math.ceil(n / 256) + 8
    return La, Lz


def gradient_bound(ref: dict, alpha: float, n: int) -> np.ndarray:
    La, Lz = gradient_depths(n)
    ba, br = (8 + La) * U32 * ref["abs_a"], (14 + La) * U32 * ref["abs_r"]
    eZ = (6 + La + Lz) * U32
    Z = ref["Z"]
    return SECOND * 4.0 * (alpha * ba + (br + np.abs(ref["r"]) * (eZ + U32)) / Z + U32 * np.abs(alpha * ref["a"] - ref["r"] / Z)) + TINY


def kl_bound(ref: dict, n: int) -> float:
    La, Lz = gradient_depths(n)
    eZ = (6 + La + Lz) * U32
    return SECOND * (U32 * (3 * ref["kl_abs"] + 4 * ref["kl_p"]) + (La + Lz) * U32 * ref["kl_abs"] + eZ + E_LOG * abs(math.log(ref["Z"]))
                     + U32 * abs(ref["kl"])) + TINY


# ------------------------------------------------------------------------------------------------ descent
def update(y, upd, gains, grad, momentum, lr, min_gain):
    """-> (y', update', gains') in the dtype of the arrays (scalars are cast to it): sklearn's _gradient_descent step."""
    dt = np.asarray(y).dtype.type
    momentum, lr, min_gain = dt(momentum), dt(lr), dt(min_gain)
    inc = upd * grad < dt(0.0)
    g2 = np.where(inc, gains + dt(0.2), gains * dt(0.8))
    g2 = np.maximum(g2, min_gain)
    gg = grad * g2
    u2 = momentum * upd - lr * gg
    return y + u2, u2, g2


def schedule(iteration: int, n: int, early_exaggeration=12.0, exaggeration_iters=250):
    early = iteration < exaggeration_iters
    return dict(momentum=0.5 if early else 0.8, alpha=early_exaggeration if early else 1.0, learning_rate=max(n / early_exaggeration / 4.0, 50.0))


def one_step(P, y, upd, gains, iteration: int, min_gain=0.01) -> dict:
    """The float64 step from a (device) state, with the bounds of the fp32 step: dict(y, update, gains, grad, y_bound, update_bound,
    exact_gains (bool mask: the sign of update * grad cannot flip), gains32 (the fp32 gains of the float64 gradient's branch: 0.2f is
    not 0.2, so "exactly" is asked of these))."""
    n = y.shape[0]
    s = schedule(iteration, n)
    y64, u64, g64 = (np.asarray(v, dtype=np.float64) for v in (y, upd, gains))
    ref = gradient(P, y64, s["alpha"])
    bg = gradient_bound(ref, s["alpha"], n)
    g = ref["grad"]
    y2, u2, gains2 = update(y64, u64, g64, g, s["momentum"], s["learning_rate"], min_gain)
    lr, mom = s["learning_rate"], s["momentum"]
    exact = (np.abs(g) > bg) | (u64 == 0.0)
    other = np.maximum(np.where(u64 * g < 0.0, g64 * 0.8, g64 + 0.2), min_gain)   # the gains of the other branch
    dG = np.where(exact, 0.0, np.abs(other - gains2))
    gmax = np.maximum(gains2, other)
    ub = SECOND * (lr * gmax * bg + lr * (np.abs(g) + bg) * dG + U32 * (np.abs(mom * u64) + 3 * lr * np.abs(g) * gmax + np.abs(u2))) + TINY
    yb = ub + SECOND * U32 * (np.abs(y2) + ub)
    g32 = np.asarray(gains, dtype=F)   # the kernel's gains in its own arithmetic, on the branch the float64 gradient takes
    gains32 = np.maximum(np.where(u64 * g < 0.0, g32 + F(0.2), g32 * F(0.8)), F(min_gain))
    return dict(y=y2, update=u2, gains=gains2, gains32=gains32, grad=g, grad_bound=bg, update_bound=ub, y_bound=yb, exact_gains=exact)


def fit(x, init, perplexity=30.0, max_iter=1000, min_gain=0.01, P=None) -> dict:
    """DeviceTSNE.fit in float64 -> dict(Z, kl)."""
    P = affinities(x, perplexity) if P is None else P
    y = np.asarray(init, dtype=np.float64).copy()
    n = y.shape[0]
    upd, gains = np.zeros_like(y), np.ones_like(y)
    off = ~np.eye(n, dtype=bool)
    for it in range(max_iter):
        s = schedule(it, n)
        diff = y[:, None, :] - y[None, :, :]
        w = 1.0 / (1.0 + (diff ** 2).sum(-1))
        Z = (w * off).sum()
        g = 4.0 * (s["alpha"] * ((P * w)[:, :, None] * diff).sum(1) - ((w * w)[:, :, None] * diff).sum(1) / Z)
        y, upd, gains = update(y, upd, gains, g, s["momentum"], s["learning_rate"], min_gain)
    return dict(Z=y, kl=gradient(P, y, 1.0)["kl"])
