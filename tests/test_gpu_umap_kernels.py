"""mae_umap_fuzzy_knn and mae_umap_epoch on the MI355X against the float64 restatement, the exact fp32 / integer restatement and the
counted bounds of tests/umap_ref.py.

Neighbours and smooth distances: the minimum shape, one dimension, tails of every tile and of the 256-thread walk, the largest k, and 8
copies of 8 points (zero distances, index ties, rows whose rho is 0).  One epoch: a ring, a hand-made graph with an empty row, a degree-1
row, a 200-edge hub row fed by repeated columns, two coincident points and negative samples that hit their own row, and the blob graph;
at y scales 1e-3 (the repulsion coefficient at its largest: most repulsions clipped), 1 and 30, at t = 0, 1, n_epochs / 2 and
n_epochs - 1, with rates 1, 5 and 16.  Every check prints worst error / bound."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import umap_ref as R

pytestmark = pytest.mark.gpu

POISON, GUARD = 777.0, 4
N_EPOCHS = 500
KNN_SHAPES = [(8, 3, 2), (65, 1, 15), (257, 5, 15), (300, 384, 64)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def _lib():
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    return lib, _ptr, _stream


def guarded(shape, dtype, dev, fill=None):
    """(buffer, view): the view sits GUARD elements inside a poisoned buffer (16 bytes: the view keeps the alignment of the buffer)."""
    count = int(np.prod(shape))
    buf = torch.full((count + 2 * GUARD,), POISON, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + count].view(shape)
    if fill is not None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(fill)).to(dev))
    return buf, view


def guards_intact(buf):
    b = buf.cpu().numpy()
    return (b[:GUARD] == POISON).all() and (b[-GUARD:] == POISON).all()


def np_(t):
    return t.detach().cpu().numpy()


@lru_cache(maxsize=None)
def ab32():
    from ssrl_vit_mae_jepa_amd.embedding import find_ab_params
    return tuple(float(np.float32(v)) for v in find_ab_params())


# ---------------------------------------------------------------------------------------------------- neighbours, rho, sigma, memberships
def fuzzy_knn(dev, x, k):
    lib, _ptr, _stream = _lib()
    n, dim = x.shape
    xd = torch.from_numpy(x).to(dev)
    bufs = {}
    for name, shape, dt in (("knn_idx", (n, k), torch.int32), ("knn_dist", (n, k), torch.float32), ("memb", (n, k), torch.float32),
                            ("rho", (n,), torch.float32), ("sigma", (n,), torch.float32)):
        bufs[name] = guarded(shape, dt, dev)
    nbytes = lib.mae_umap_scratch_bytes(n, dim, k)
    assert nbytes > 0
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.mae_umap_fuzzy_knn(_ptr(xd), n, dim, k, *(_ptr(bufs[name][1]) for name in ("knn_idx", "knn_dist", "memb", "rho", "sigma")), _ptr(scratch), nbytes,
                                _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.mae_last_error()
    for name, (buf, _) in bufs.items():
        assert guards_intact(buf), f"{name}: a guard element was written"
    return {name: np_(view).copy() for name, (_, view) in bufs.items()}


def check_fuzzy_knn(dev, x, k, tag):
    n, dim = x.shape
    out = fuzzy_knn(dev, x, k)
    idx, dist, memb, rho, sigma = (out[v] for v in ("knn_idx", "knn_dist", "memb", "rho", "sigma"))
    D64 = np.sqrt(R.sqdist(x))
    bound = R.knn_dist_bound(D64, dim)
    rows = np.arange(n)[:, None]
    fails = []
    # the lists: valid, distinct, each distance that of its index, sorted by (distance, index), nothing closer left out
    assert idx.min() >= 0 and idx.max() < n and all(len(set(r)) == k for r in idx.tolist())
    rd = np.abs(dist.astype(np.float64) - D64[rows, idx]) / bound[rows, idx]
    if not rd.max() <= 1.0:
        fails.append(f"knn_dist error / bound {rd.max():.3g} at {np.unravel_index(rd.argmax(), rd.shape)}")
    step = np.diff(dist, axis=1)
    assert (step >= 0).all() and (np.diff(idx, axis=1)[step == 0] > 0).all(), "a row is not sorted by (distance, index)"
    left = np.ones((n, n), dtype=bool)
    left[rows, idx] = False
    kth = D64[np.arange(n), idx[:, -1]]
    gap = np.where(left, (kth[:, None] - D64) - (bound + bound[np.arange(n), idx[:, -1]][:, None]), -np.inf)
    if not gap.max() <= 0.0:
        fails.append(f"a left-out point is closer than the k-th entry by {gap.max():.3g} more than the bound at {np.unravel_index(gap.argmax(), gap.shape)}")
    # rho: exactly the first non-zero entry
    nz = dist > 0
    want_rho = np.where(nz.any(1), dist[np.arange(n), nz.argmax(1)], np.float32(0))
    assert (rho.view(np.uint32) == want_rho.view(np.uint32)).all(), "rho is not the first non-zero entry"
    # sigma: the float64 sum on the device's own distances at the device's own sigma, or the floor
    assert np.isfinite(sigma).all() and (sigma > 0).all()
    ps, slack = R.smooth_sum(dist, rho, sigma)
    off = np.abs(ps - np.log2(k)) > R.TOL + slack
    d64 = dist.astype(np.float64)
    floor = R.FLOOR * np.where(rho > 0, d64.mean(1), d64.mean())
    floor_tol = R.SECOND * (np.ceil(n / 256) + 20 + k) * R.U32 * floor + R.TINY
    held = np.abs(sigma - floor) <= floor_tol
    assert (sigma >= floor - floor_tol).all(), "a sigma lies below its floor"
    if (off & ~held).any():   # a row may stop unconverged only after 64 steps, and then the float64 search of the same row needed them too
        ref = R.smooth(d64)
        bad = off & ~held & (ref["steps"] < R.SEARCH_STEPS)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            fails.append(f"{int(bad.sum())} rows off log2 k: row {i} sum {ps[i]!r} vs {np.log2(k)!r}, slack {slack[i]:.3g}, sigma {sigma[i]!r}, floor {floor[i]!r}")
    m64, mb = R.memberships(idx, dist, rho, sigma)
    rm = np.abs(memb.astype(np.float64) - m64) / np.where(mb > 0, mb, 1.0)
    exact = mb == 0
    assert (memb[exact] == m64[exact]).all(), "a membership that is exactly 0 or 1 is not"
    if not rm[~exact].max(initial=0.0) <= 1.0:
        fails.append(f"memb error / bound {rm[~exact].max():.3g}")
    free = ~off
    print(f"{tag}: knn_dist {rd.max():.3g} memb {rm[~exact].max(initial=0.0):.3g} of their bounds; worst |sum - log2 k| where the floor is not held "
          f"{np.abs(ps - np.log2(k))[free].max(initial=0.0):.3g} (slack {slack.max():.2g}); {int(held.sum())} rows on the floor, {int((rho == 0).sum())} with rho = 0")
    assert not fails, "\n".join(fails)
    again = fuzzy_knn(dev, x, k)
    for name in out:
        assert (out[name].view(np.uint32) == again[name].view(np.uint32)).all(), f"{name} differs between two calls"
    return out


@pytest.mark.parametrize("n,dim,k", KNN_SHAPES)
def test_fuzzy_knn(dev, n, dim, k):
    out = check_fuzzy_knn(dev, R.gen_features(n, dim), k, f"({n}, {dim}, {k})")
    assert (out["knn_idx"][:, 0] == np.arange(n)).all() and (out["knn_dist"][:, 0] == 0).all()   # no duplicates: the point itself is entry 0
    assert (out["memb"][:, 0] == 0).all() and (out["memb"][:, 1] == 1).all()


@pytest.mark.parametrize("k", [5, 15])
def test_fuzzy_knn_on_copies(dev, k):
    out = check_fuzzy_knn(dev, R.copies(), k, f"8 copies of 8 points, k = {k}")
    same = np.arange(64)[:, None] % 8 + 8 * np.arange(8)[None, :]          # the 8 copies of a row's point, index ascending
    assert (out["knn_idx"][:, :min(k, 8)] == same[:, :min(k, 8)]).all() and (out["knn_dist"][:, :min(k, 8)] == 0).all()
    own = out["knn_idx"] == np.arange(64)[:, None]
    assert (out["memb"][own] == 0).all() and (out["memb"][:, :min(k, 8)][~own[:, :min(k, 8)]] == 1).all()
    assert ((out["rho"] == 0).all() and (own.sum(1) == (np.arange(64) < 40)).all()) if k == 5 else (out["rho"] > 0).all()


# ---------------------------------------------------------------------------------------------------- one epoch
def _csr(n, lists, seed):
    r = np.random.default_rng([n, seed, 17])
    row_ptr = np.zeros(n + 1, dtype=np.int32)
    row_ptr[1:] = np.cumsum([len(c) for c in lists])
    col = np.concatenate([np.asarray(c, dtype=np.int32) for c in lists]) if row_ptr[-1] else np.zeros(0, dtype=np.int32)
    eps = (1.0 + 5.0 * r.random(len(col)) ** 2).astype(np.float32)
    eps[:: 3] = 1.0
    return dict(n=n, row_ptr=row_ptr, col=col, eps=eps)


@lru_cache(maxsize=None)
def graph(name):
    if name == "ring":
        return _csr(8, [sorted(((i - 1) % 8, (i + 1) % 8)) for i in range(8)], 0)
    if name == "crafted":
        r = np.random.default_rng(70)
        lists = [sorted(r.choice(70, size=int(r.integers(3, 9)), replace=False).tolist()) for _ in range(70)]
        lists[0] = []                                            # an empty row
        lists[1] = [40]                                          # degree 1
        lists[2] = sorted((np.arange(200) % 70).tolist())        # a hub: 200 edges, repeated columns
        lists[5] = sorted(set(lists[5]) | {6})                   # rows 5 and 6 coincide, and are joined
        lists[6] = sorted(set(lists[6]) | {5})
        return _csr(70, lists, 1)
    x, _ = R.blobs()
    g = R.graph_of(x, 15, N_EPOCHS, np.float32)
    return dict(n=600, row_ptr=g["row_ptr"], col=g["col"], eps=g["eps"])


def positions(g, scale):
    y = (scale * np.random.default_rng([g["n"], 19]).standard_normal((g["n"], 2))).astype(np.float32)
    if g["n"] == 70:
        y[6] = y[5]
    return y


def schedule_state(g, t):
    """next at the start of epoch t: eps itself at t = 0; else spread around t, with entries exactly t (fires) and just above (does not)."""
    if t == 0:
        return g["eps"].copy()
    nxt = np.random.default_rng([g["n"], t, 23]).uniform(0.0, 2.0 * t + 2.0, len(g["col"])).astype(np.float32)
    nxt[::7] = np.float32(t)
    nxt[3::7] = np.nextafter(np.float32(t), np.float32(np.inf))
    return nxt


def run_epoch(dev, g, y, nxt, alpha, t, rate, seed):
    lib, _ptr, _stream = _lib()
    a, b = ab32()
    n = g["n"]
    yin_buf, yin = guarded((n, 2), torch.float32, dev, y)
    yout_buf, yout = guarded((n, 2), torch.float32, dev)
    next_buf, nx = guarded((len(nxt),), torch.float32, dev, nxt)
    row_ptr, col, eps = (torch.from_numpy(g[v]).to(dev) for v in ("row_ptr", "col", "eps"))
    rc = lib.mae_umap_epoch(_ptr(yin), _ptr(yout), _ptr(row_ptr), _ptr(col), _ptr(eps), _ptr(nx), n, a, b, 1.0, alpha, t, rate, seed, _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.mae_last_error()
    assert guards_intact(yin_buf) and guards_intact(yout_buf) and guards_intact(next_buf), "a guard element was written"
    assert (np_(yin).view(np.uint32) == y.view(np.uint32)).all(), "y_in was written"
    assert (np_(eps) == g["eps"]).all() and (np_(col) == g["col"]).all()
    return np_(yout).copy(), np_(nx).copy()


@pytest.mark.parametrize("scale", [1e-3, 1.0, 30.0])
@pytest.mark.parametrize("name", ["ring", "crafted", "blobs"])
def test_epoch(dev, name, scale):
    g = graph(name)
    a, b = ab32()
    y = positions(g, scale)
    rows = np.repeat(np.arange(g["n"]), np.diff(g["row_ptr"]))
    seed, worst, fired, own = 73, 0.0, 0, 0
    for t in (0, 1, N_EPOCHS // 2, N_EPOCHS - 1):
        nxt = schedule_state(g, t)
        alpha = R.alpha_of(t, N_EPOCHS)
        for rate in (1, 5, 16):
            got_y, got_next = run_epoch(dev, g, y, nxt, alpha, t, rate, seed)
            ref = R.epoch(y, g["row_ptr"], g["col"], g["eps"], nxt, a, b, 1.0, alpha, t, rate, seed)
            assert (got_next.view(np.uint32) == ref["next"].view(np.uint32)).all(), f"t {t} rate {rate}: next differs from the fp32 restatement"
            if t == 0:
                assert not ref["active"].any() and (got_y.view(np.uint32) == y.view(np.uint32)).all(), "t = 0: nothing fires, y_out is y_in"
            ratio = np.abs(got_y.astype(np.float64) - ref["y"]) / ref["bound"]
            assert ratio.max() <= 1.0, f"t {t} rate {rate}: y_out error / bound {ratio.max():.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
            worst = max(worst, float(ratio.max()))
            fired += int(ref["active"].sum())
            own += int((ref["negatives"] == rows[ref["active"]][:, None]).sum())
            again_y, again_next = run_epoch(dev, g, y, nxt, alpha, t, rate, seed)
            assert (again_y.view(np.uint32) == got_y.view(np.uint32)).all() and (again_next.view(np.uint32) == got_next.view(np.uint32)).all()
    print(f"{name} scale {scale:g}: worst y_out error / bound {worst:.3g}; {fired} firings, {own} negative samples on their own row")
    assert fired > 0
    if name == "crafted":
        assert own > 0   # the k = i case has been met


def test_epoch_depends_on_seed_and_epoch_only_through_the_negatives(dev):
    g, y = graph("crafted"), positions(graph("crafted"), 1.0)
    nxt = schedule_state(g, 250)
    base, _ = run_epoch(dev, g, y, nxt, 0.5, 250, 5, 73)
    other, _ = run_epoch(dev, g, y, nxt, 0.5, 250, 5, 74)
    assert (base != other).any() and (base[0] == y[0]).all() and (other[0] == y[0]).all()   # the empty row stays


@pytest.mark.parametrize("args,word", [((7, 1.0, 1.0, 1.0, 1.0, 0, 5), "n = 7"), ((16385, 1.0, 1.0, 1.0, 1.0, 0, 5), "n = 16385"),
                                       ((100, 1.0, 1.0, 1.0, 1.0, 0, 0), "negative_sample_rate = 0"), ((100, 1.0, 1.0, 1.0, 1.0, -1, 5), "t = -1")])
def test_epoch_refusals_name_the_limit(dev, args, word):
    lib, _, _ = _lib()
    assert lib.mae_umap_epoch(None, None, None, None, None, None, *args, 73, None) != 0
    assert word in lib.mae_last_error().decode()


def test_epoch_in_place_and_short_scratch_are_refused(dev):
    lib, _ptr, _stream = _lib()
    g = graph("ring")
    y = torch.full((8, 2), POISON, dtype=torch.float32, device=dev)
    row_ptr, col, eps = (torch.from_numpy(g[v]).to(dev) for v in ("row_ptr", "col", "eps"))
    nxt = eps.clone()
    assert lib.mae_umap_epoch(_ptr(y), _ptr(y), _ptr(row_ptr), _ptr(col), _ptr(eps), _ptr(nxt), 8, 1.0, 1.0, 1.0, 1.0, 3, 5, 73, _stream(dev)) != 0
    assert b"y_out must not be y_in" in lib.mae_last_error()
    x = torch.zeros((65, 4), dtype=torch.float32, device=dev)
    out = [torch.full((65, 15), POISON, dtype=torch.float32, device=dev) for _ in range(2)]
    idx = torch.full((65, 15), 777, dtype=torch.int32, device=dev)
    rs = [torch.full((65,), POISON, dtype=torch.float32, device=dev) for _ in range(2)]
    nbytes = lib.mae_umap_scratch_bytes(65, 4, 15)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.mae_umap_fuzzy_knn(_ptr(x), 65, 4, 15, _ptr(idx), _ptr(out[0]), _ptr(out[1]), _ptr(rs[0]), _ptr(rs[1]), _ptr(scratch), nbytes - 4, _stream(dev))
    torch.cuda.synchronize()
    assert rc != 0 and b"scratch_bytes" in lib.mae_last_error()
    assert (np_(y) == POISON).all() and (np_(out[0]) == POISON).all() and (np_(idx) == 777).all() and (np_(nxt) == g["eps"]).all()
