"""float64 numpy restatement of the UMAP kernels (k_umap.hip) and of embedding.DeviceUMAP, the exact fp32 / integer restatement of what
the device must reproduce bit for bit (the fuzzy union, eps, the `next` schedule, the negative indices), the per-element error bounds of
the fp32 kernels against the float64 reference, trustworthiness, and the data of the tests.  numpy only.

Reference (steps as in DESIGN.md 11.4)
  knn(x, k)                         d = sqrt(sum_c (x_ic - x_jc)^2); per row the k smallest by (distance, index), the point itself included
  smooth(dist)                      umap-learn's smooth_knn_dist: rho, sigma (with the two floors), steps, which rows the floor raised
  smooth_sum(dist, rho, sigma)      sum_{r = 1 .. k - 1} e^(-max(d_r - rho, 0) / sigma) per row
  memberships(idx, dist, rho, sigma)
  fuzzy_union(idx, memb, n_epochs)  W = (A + A^T) - (A * A^T) in the dtype of memb, each operation rounded once; edges below max / n_epochs
                                    dropped; CSR over both directions, columns ascending; eps = max / w.  With float32 memberships this is
                                    the device's graph bit for bit.
  negative_index(seed, t, e, s, n)  the kernel's integer formula in numpy uint64 masked to 32 bits
  epoch(...)                        one synchronous epoch in float64 from given positions, with the fp32 restatement of the active set and
                                    of next, the negative indices, and the bound of the fp32 kernel's y_out
  fit(x, ...)                       the whole DeviceUMAP.fit in float64 (eps and next in fp32, as on the device)
  trustworthiness(X, Z, k)          sklearn.manifold.trustworthiness, restated

Bounds, first order, counted from the kernel's statements.  u = 2^-24; E_EXP = E_LOG = E_SQRT = 2 u: one ulp of v_exp_f32, v_log_f32 /
log2f, exp2f and of the square root (taken from the ISA manual and the ocml, as tests/tsne_ref.py does, not measured); SECOND = 1 + 2^-6
covers products of first-order terms; TINY = 2^-120 results flushed below the normal range.
  knn_dist  d2 carries (dim + 2) u (tests/tsne_ref.py), the root halves it and adds E_SQRT:   ((dim + 2) / 2 + 2) u d
  psum      X_r = (d_r - rho) / mid: the difference rounds (u X), the quotient rounds (u X), __expf multiplies by a rounded log2 e and
            rounds the product (2 u X), v_exp_f32 E_EXP: a term carries eE_r = 4 u X_r + E_EXP.  Six butterfly levels (6 u psum), the
            rounded target (u log2 k):   slack = sum_r e_r eE_r + 6 u psum + u log2 k
  memb      against float64 on the device's own d, rho, sigma: the same term:   m (4 u X + E_EXP)
  epoch     dx = fl(y_i - y_o): u.  d2 = fma(dx, dx, fl(dy dy)): <= 4 u.  L = log2f(d2): 4 u / ln 2 from d2 and E_LOG |L|; b L rounds
            (u b |L|); exp2f E_EXP:   pb = d2^b carries  ePB = (4 b + 2) u + 3 u b |ln d2|.
            attraction: pb / d2 (ePB + 5 u), times fl(-2 fl(a b)) (2 u), den = fma(a, pb, 1) (ePB + 2 u), the quotient (u), times dx
            (2 u):   2 ePB + 12 u.   repulsion: fl(0.001f + d2) (6 u), den (ePB + 2 u), their product (u), fl(2 fl(gamma b)) and the
            quotient (2 u), times dx (2 u):   ePB + 13 u.   clip is 1-Lipschitz: a term's error survives it at most unchanged, and is 0
            when the term lies beyond the clip by more than its error.  A lane adds ceil(degree / E) terms in order, E = floor(64 /
            (rate + 1)), then six butterfly levels: depth = ceil(degree / E) + 6 roundings, each <= u sum |terms|.  y' = fma(alpha, sum,
            y) rounds once:   alpha (sum_terms err + depth u sum |terms|) + u |y'|.
"""
from __future__ import annotations

import math

import numpy as np

from tests.tsne_ref import blobs, loo_1nn_accuracy, sqdist  # noqa: F401  (the blob data and the difference-form distances are shared)

U32 = 2.0 ** -24
E_EXP = E_LOG = E_SQRT = 2 * U32
SECOND = 1.0 + 2.0 ** -6
TINY = 2.0 ** -120
SEARCH_STEPS, TOL, FLOOR = 64, 1e-5, 1e-3
F = np.float32
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ data
def gen_features(n: int, dim: int, seed: int = 0) -> np.ndarray:
    r = np.random.default_rng([n, dim, seed, 7])
    return (r.standard_normal((n, dim)) + 2.0 * r.standard_normal((3, dim))[r.integers(0, 3, n)]).astype(F)


def copies(points: int = 8, times: int = 8, dim: int = 5, seed: int = 0) -> np.ndarray:
    """points x times rows: every point `times` times, interleaved -- zero distances, index ties, rows whose rho is 0 for k <= times."""
    r = np.random.default_rng([points, times, dim, seed])
    return np.tile(r.standard_normal((points, dim)), (times, 1)).astype(F)


# ------------------------------------------------------------------------------------------------ neighbours and smooth distances
def knn(x, k: int):
    """-> (idx (n, k) int64, dist (n, k) float64, D (n, n) float64 distances)."""
    D = np.sqrt(sqdist(x))
    n = D.shape[0]
    idx = np.empty((n, k), dtype=np.int64)
    for i in range(n):
        idx[i] = np.lexsort((np.arange(n), D[i]))[:k]   # by distance, then by index
    return idx, np.take_along_axis(D, idx, 1), D


def knn_dist_bound(d64, dim: int):
    return SECOND * ((dim + 2) / 2.0 + 2.0) * U32 * d64 + TINY


def _psum(d, rho, mid):
    dd = d[1:] - rho
    return float(np.where(dd > 0, np.exp(-np.maximum(dd, 0.0) / mid), 1.0).sum())


def smooth(dist):
    """dist (n, k) -> dict(rho, sigma, steps, floored (bool), psum at sigma before the floor)."""
    dist = np.asarray(dist, dtype=np.float64)
    n, k = dist.shape
    target = math.log2(k)
    rho, sigma, steps, floored = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    mean_all = dist.mean()
    for i in range(n):
        nz = dist[i][dist[i] > 0]
        rho[i] = nz[0] if len(nz) else 0.0
        lo, hi, mid = 0.0, np.inf, 1.0
        step = 0
        for step in range(SEARCH_STEPS):
            ps = _psum(dist[i], rho[i], mid)
            if abs(ps - target) < TOL:
                break
            if ps > target:
                hi = mid
                mid = (lo + hi) / 2.0
            else:
                lo = mid
                mid = mid * 2.0 if hi == np.inf else (lo + hi) / 2.0
        else:
            step = SEARCH_STEPS
        steps[i] = min(step + 1, SEARCH_STEPS)
        floor = FLOOR * (dist[i].mean() if rho[i] > 0 else mean_all)
        floored[i] = mid < floor
        sigma[i] = max(mid, floor)
    return dict(rho=rho, sigma=sigma, steps=steps, floored=floored)


def smooth_sum(dist, rho, sigma):
    """-> (psum (n), slack (n)): the float64 sum at the given sigma and the counted slack of the fp32 sum."""
    dist, rho, sigma = (np.asarray(v, dtype=np.float64) for v in (dist, rho, sigma))
    k = dist.shape[1]
    dd = np.maximum(dist[:, 1:] - rho[:, None], 0.0)
    X = dd / sigma[:, None]
    e = np.where(dd > 0, np.exp(-X), 1.0)
    eE = np.where(dd > 0, 4 * U32 * X + E_EXP, 0.0)
    ps = e.sum(1)
    return ps, SECOND * ((e * eE).sum(1) + 6 * U32 * ps + U32 * math.log2(k))


def memberships(idx, dist, rho, sigma):
    """-> (memb (n, k) float64, bound (n, k))."""
    dist, rho, sigma = (np.asarray(v, dtype=np.float64) for v in (dist, rho, sigma))
    n = dist.shape[0]
    dd = dist - rho[:, None]
    one = (dd <= 0) | (sigma[:, None] == 0)
    X = np.where(one, 0.0, dd / np.where(sigma[:, None] == 0, 1.0, sigma[:, None]))
    m = np.where(one, 1.0, np.exp(-X))
    own = np.asarray(idx) == np.arange(n)[:, None]
    m[own] = 0.0
    return m, np.where(one | own, 0.0, SECOND * m * (4 * U32 * X + E_EXP) + TINY)


# ------------------------------------------------------------------------------------------------ the graph
def fuzzy_union(idx, memb, n_epochs: int):
    """-> dict(row_ptr (n + 1) int32, col (E) int32, w (E), eps (E) float32, wmax) in the dtype of memb (float32: the device's bits)."""
    memb = np.asarray(memb)
    dt = memb.dtype.type
    n, k = memb.shape
    A = np.zeros((n, n), dtype=memb.dtype)
    A[np.arange(n)[:, None], np.asarray(idx)] = memb
    W = (A + A.T) - (A * A.T)
    wmax = W.max()
    W[W < wmax / dt(n_epochs)] = 0
    rows, cols = np.nonzero(W)   # row-major: columns ascend within a row
    w = W[rows, cols]
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return dict(row_ptr=row_ptr, col=cols.astype(np.int32), w=w, eps=(wmax / w).astype(F), wmax=wmax, W=W, rows=rows.astype(np.int32))


# ------------------------------------------------------------------------------------------------ the generator
def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & M32
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & M32
    h ^= h >> np.uint64(16)
    return h


def mix(seed, i):
    i = (np.asarray(i, dtype=np.uint64) + np.uint64(0x9E3779B9)) & M32
    return fmix32(fmix32(i) ^ (np.asarray(seed, dtype=np.uint64) & M32))


def negative_index(seed: int, t: int, e, s, n: int):
    """k = (uint64(h) n) >> 32, h = mix(mix(seed, t), 16 e + s): e the edge's index in col, s the sample."""
    key = (np.uint64(16) * np.asarray(e, dtype=np.uint64) + np.asarray(s, dtype=np.uint64)) & M32
    h = mix(mix(seed, t), key)
    return ((h * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def next_update(nxt, eps, t: int):
    """fp32, bit for bit: -> (active (E) bool, next')."""
    nxt, eps = np.asarray(nxt, dtype=F), np.asarray(eps, dtype=F)
    active = nxt <= F(t)
    return active, np.where(active, nxt + eps, nxt).astype(F)


# ------------------------------------------------------------------------------------------------ the layout
def _clip_term(c, diff, rel):
    """c (m), diff (m, 2), rel (m) -> (clip(c diff), |clip|, the error that survives the clip), each (m, 2)."""
    x = c[:, None] * diff
    g = np.clip(x, -4.0, 4.0)
    err = np.where(np.abs(x) * (1.0 - rel[:, None]) > 4.0, 0.0, rel[:, None] * np.abs(x))
    return g, np.abs(g), err


def epoch(y, row_ptr, col, eps, nxt, a: float, b: float, gamma: float, alpha: float, t: int, rate: int, seed: int):
    """One synchronous epoch in float64 from y (n, 2) -> dict(y, next, active, negatives (E_active, rate), bound (n, 2))."""
    y = np.asarray(y, dtype=np.float64)
    n = y.shape[0]
    row_ptr, col = np.asarray(row_ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(row_ptr))
    active, nxt2 = next_update(nxt, eps, t)
    e = np.nonzero(active)[0]
    ri = rows[e]
    acc, mag, err = np.zeros_like(y), np.zeros_like(y), np.zeros_like(y)

    def pb_of(d2):
        safe = np.where(d2 > 0, d2, 1.0)
        return np.power(safe, b), (4 * b + 2) * U32 + 3 * U32 * b * np.abs(np.log(safe))

    diff = y[ri] - y[col[e]]
    d2 = (diff ** 2).sum(1)
    pb, ePB = pb_of(d2)
    c = np.where(d2 > 0, -2.0 * a * b * (pb / np.where(d2 > 0, d2, 1.0)) / (a * pb + 1.0), 0.0)
    g, m, er = _clip_term(c, diff, 2 * ePB + 12 * U32)
    np.add.at(acc, ri, 2.0 * g)
    np.add.at(mag, ri, 2.0 * m)
    np.add.at(err, ri, 2.0 * er)
    neg = np.empty((len(e), rate), dtype=np.int64)
    for s in range(rate):
        k = negative_index(seed, t, e, s, n)
        neg[:, s] = k
        diff = y[ri] - y[k]
        d2 = (diff ** 2).sum(1)
        pb, ePB = pb_of(d2)
        c = np.where((d2 > 0) & (k != ri), 2.0 * gamma * b / ((0.001 + d2) * (a * pb + 1.0)), 0.0)
        g, m, er = _clip_term(c, diff, ePB + 13 * U32)
        np.add.at(acc, ri, g)
        np.add.at(mag, ri, m)
        np.add.at(err, ri, er)
    y2 = y + alpha * acc
    depth = np.ceil(np.diff(row_ptr) / (64 // (rate + 1))) + 6
    bound = SECOND * (alpha * (err + depth[:, None] * U32 * mag) + U32 * np.abs(y2)) + TINY
    return dict(y=y2, next=nxt2, active=active, negatives=neg, bound=bound)


def default_epochs(n: int) -> int:
    return 500 if n <= 10000 else 200


def alpha_of(t: int, n_epochs: int, learning_rate: float = 1.0) -> float:
    """The epoch's step, rounded to fp32 on the host as DeviceUMAP rounds it."""
    return float(F(learning_rate * (1.0 - t / n_epochs)))


def graph_of(x, k: int = 15, n_epochs: int = None, dtype=np.float64):
    """Steps 1 - 3 in float64 (dtype float32: the union in fp32 from the rounded memberships) -> fuzzy_union's dict plus idx, dist."""
    idx, dist, _ = knn(x, k)
    s = smooth(dist)
    m, _ = memberships(idx, dist, s["rho"], s["sigma"])
    g = fuzzy_union(idx, m.astype(dtype), n_epochs or default_epochs(len(idx)))
    g.update(idx=idx, dist=dist, memb=m, **s)
    return g


def fit(x, init, a: float, b: float, k: int = 15, n_epochs: int = None, rate: int = 5, learning_rate: float = 1.0, gamma: float = 1.0, seed: int = 73,
        graph=None):
    """DeviceUMAP.fit in float64 -> dict(Z, graph)."""
    n = len(init)
    n_epochs = n_epochs or default_epochs(n)
    g = graph or graph_of(x, k, n_epochs)
    y, nxt = np.asarray(init, dtype=np.float64).copy(), g["eps"].copy()
    for t in range(n_epochs):
        out = epoch(y, g["row_ptr"], g["col"], g["eps"], nxt, a, b, gamma, alpha_of(t, n_epochs, learning_rate), t, rate, seed)
        y, nxt = out["y"], out["next"]
    return dict(Z=y, graph=g)


# ------------------------------------------------------------------------------------------------ quality
def trustworthiness(X, Z, k: int = 15) -> float:
    """sklearn.manifold.trustworthiness (Euclidean): 1 - 2 / (n k (2 n - 3 k - 1)) sum_i sum_{j in the k nearest of i in Z} max(rank_X(i, j) - k, 0)."""
    DX, DZ = np.sqrt(sqdist(X)), np.sqrt(sqdist(Z))
    n = DX.shape[0]
    np.fill_diagonal(DX, np.inf)
    np.fill_diagonal(DZ, np.inf)
    order = np.argsort(DX, axis=1, kind="stable")
    rank = np.empty((n, n), dtype=np.int64)
    rank[np.arange(n)[:, None], order] = np.arange(1, n + 1)[None, :]
    near = np.argsort(DZ, axis=1, kind="stable")[:, :k]
    r = np.take_along_axis(rank, near, 1) - k
    return 1.0 - float(r[r > 0].sum()) * 2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0))
