"""mae_tsne_affinities, mae_tsne_gradient, mae_tsne_update and mae_tsne_step on the MI355X against the float64 restatement and the
counted bounds of tests/tsne_ref.py: at n below, at and above the 64-wide tiles and the 256-thread strides, with n no multiple of 4
(padded pitch), identical rows, a far outlier, the perplexity's ends, y at the initial and at late scales, exact zeros in P."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from tests import tsne_ref as T

pytestmark = pytest.mark.gpu

NS = (8, 63, 65, 257, 1030)
DIMS = (4, 100, 384)
POISON = 777.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


def _lib():
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    return lib, _ptr, _stream


def perplexities(n):
    """2, 30 where n admits it, and the largest admitted: the fp32 value just below n - 1."""
    top = float(np.nextafter(np.float32(n - 1), np.float32(0)))
    return [p for p in (2.0, 30.0) if p < n - 1] + [top]


@lru_cache(maxsize=None)
def features(n, dim, case="plain"):
    x = T.gen_features(n, dim, case=case)
    return x, T.sqdist(x)


def affinities(dev, x, perp):
    lib, _ptr, _stream = _lib()
    n, dim = x.shape
    pitch = lib.mae_tsne_pitch(n)
    xd = torch.from_numpy(x).to(dev)
    P = torch.full((n, pitch), POISON, dtype=torch.float32, device=dev)
    sq, pc = (torch.full((n, n), POISON, dtype=torch.float32, device=dev) for _ in range(2))
    beta = torch.full((n + 4,), POISON, dtype=torch.float32, device=dev)
    rc = lib.mae_tsne_affinities(_ptr(xd), n, dim, perp, _ptr(P), _ptr(sq), _ptr(beta), _ptr(pc), _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.mae_last_error()
    return dict(P=P, sqdist=sq, beta=beta, p_cond=pc, pitch=pitch)


def check_affinities(dev, x, D64, perp, tag):
    n, dim = x.shape
    out = affinities(dev, x, perp)
    sq, beta, pc, P = np_(out["sqdist"]), np_(out["beta"]), np_(out["p_cond"]), np_(out["P"])
    fails = []
    # distances: per element against float64, symmetric bit for bit, zero diagonal
    ratio = np.abs(sq.astype(np.float64) - D64) / T.sqdist_bound(D64, dim)
    if not ratio.max() <= 1.0:
        fails.append(f"sqdist error / bound {ratio.max():.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)}")
    assert (sq == sq.T).all() and (np.diag(sq) == 0).all()
    assert (beta[n:] == POISON).all() and np.isfinite(beta[:n]).all() and (beta[:n] > 0).all()
    # the search, on the device's own distances at the device's own beta
    Dd, b = sq.astype(np.float64), beta[:n].astype(np.float64)
    pb, slack = T.search_bounds(Dd, b, perp)
    H = T.entropy(Dd, b)
    miss = np.abs(H - np.log(perp)) > T.TOL + slack
    if miss.any():   # a row may stop unconverged only after 100 steps, and then the float64 search of the same row needed them too
        ref = T.search(Dd, perp)
        bad = miss & (ref["steps"] < T.MAX_STEPS)
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            fails.append(f"{int(bad.sum())} rows off the perplexity: row {i} H {H[i]!r} vs {np.log(perp)!r}, slack {slack[i]:.3g}, beta {b[i]!r}")
    pr = np.abs(pc.astype(np.float64) - T.softmax(Dd, b)) / np.where(pb > 0, pb, 1.0)
    if not pr.max() <= 1.0:
        fails.append(f"p_cond error / bound {pr.max():.3g} at {np.unravel_index(pr.argmax(), pr.shape)}")
    assert (np.diag(pc) == 0).all()
    # the joint matrix: exact fp32 arithmetic on p_cond
    want = (pc + pc.T) / np.float32(2 * n)
    assert (P[:, :n] == want).all(), "P is not fl(fl(p_j|i + p_i|j) / 2n)"
    assert (P[:, :n] == P[:, :n].T).all() and (np.diag(P) == 0).all() and (P[:, n:] == 0).all()
    sum_bound = pb.sum() / n + 2 * T.U32
    total = P[:, :n].astype(np.float64).sum()
    if not abs(total - 1.0) <= sum_bound:
        fails.append(f"sum of P {total!r}: off 1 by more than {sum_bound:.3g}")
    print(f"{tag} perplexity {perp:g}: sqdist {ratio.max():.3g} p_cond {pr.max():.3g} of their bounds; worst |H - log perp| {np.abs(H - np.log(perp)).max():.3g} "
          f"(slack {slack.max():.2g}); |sum P - 1| {abs(total - 1):.2g}")
    assert not fails, "\n".join(fails)
    # twice the same bits
    again = affinities(dev, x, perp)
    for k in ("P", "sqdist", "beta", "p_cond"):
        assert torch.equal(out[k], again[k]), f"{k} differs between two calls"


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dim", DIMS)
def test_affinities(dev, n, dim):
    x, D64 = features(n, dim)
    for perp in perplexities(n):
        check_affinities(dev, x, D64, perp, f"({n}, {dim})")


@pytest.mark.parametrize("n,dim,case", [(65, 100, "twins"), (257, 4, "twins"), (65, 100, "outlier"), (257, 4, "outlier")])
def test_affinities_twins_and_outlier(dev, n, dim, case):
    x, D64 = features(n, dim, case)
    for perp in (2.0, 30.0):
        check_affinities(dev, x, D64, perp, f"({n}, {dim}) {case}")


def test_affinities_optional_outputs_do_not_change_p(dev):
    lib, _ptr, _stream = _lib()
    x, _ = features(65, 100)
    full = affinities(dev, x, 30.0)
    P = torch.full((65, full["pitch"]), POISON, dtype=torch.float32, device=dev)
    assert lib.mae_tsne_affinities(_ptr(torch.from_numpy(x).to(dev)), 65, 100, 30.0, _ptr(P), None, None, None, _stream(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(P, full["P"])


# ---------------------------------------------------------------------------------------------------- gradient and KL
@lru_cache(maxsize=None)
def sparse_joint(n):
    """A symmetric fp32 P with a zero diagonal, about a third exact zeros, summing to 1 up to fp32 rounding; padded to the pitch."""
    r = np.random.default_rng([n, 11])
    A = r.random((n, n)) ** 4
    A[r.random((n, n)) < 0.2] = 0.0
    A = np.triu(A, 1)
    A = A + A.T
    P = (A / A.sum()).astype(np.float32)
    padded = np.zeros((n, T.pitch_of(n)), dtype=np.float32)
    padded[:, :n] = P
    return P, padded


def gradient(dev, padded, y, alpha, want_kl=True):
    lib, _ptr, _stream = _lib()
    n = y.shape[0]
    Pd, yd = torch.from_numpy(padded).to(dev), torch.from_numpy(y).to(dev)
    grad = torch.full((n, 2), POISON, dtype=torch.float32, device=dev)
    kl = torch.full((4,), POISON, dtype=torch.float32, device=dev)
    nbytes = lib.mae_tsne_scratch_bytes(n, 1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    rc = lib.mae_tsne_gradient(_ptr(Pd), _ptr(yd), n, alpha, _ptr(grad), _ptr(kl) if want_kl else None, _ptr(scratch), nbytes, _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0, lib.mae_last_error()
    return grad, kl


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
@pytest.mark.parametrize("alpha", [1.0, 12.0])
def test_gradient_and_kl(dev, n, scale, alpha):
    P, padded = sparse_joint(n)
    y = (scale * np.random.default_rng([n, 12]).standard_normal((n, 2))).astype(np.float32)
    grad, kl = gradient(dev, padded, y, alpha)
    ref = T.gradient(P, y, alpha)
    ratio = np.abs(np_(grad).astype(np.float64) - ref["grad"]) / T.gradient_bound(ref, alpha, n)
    kr = abs(float(kl[0]) - ref["kl"]) / T.kl_bound(ref, n)
    print(f"n {n} scale {scale:g} alpha {alpha:g}: grad error / bound {ratio.max():.3g}, KL {float(kl[0])!r} vs {ref['kl']!r}: {kr:.3g} of its bound")
    assert ratio.max() <= 1.0, f"grad error / bound {ratio.max():.3g} at {np.unravel_index(ratio.argmax(), ratio.shape)}"
    assert kr <= 1.0
    assert (np_(kl)[1:] == POISON).all()
    g2, kl2 = gradient(dev, padded, y, alpha)
    assert torch.equal(grad, g2) and torch.equal(kl, kl2)
    g3, kl3 = gradient(dev, padded, y, alpha, want_kl=False)   # the same bits without the KL pass; nothing written
    assert torch.equal(grad, g3) and (np_(kl3) == POISON).all()


def test_gradient_ignores_what_the_padding_columns_hold(dev):
    P, padded = sparse_joint(65)
    y = np.random.default_rng(1).standard_normal((65, 2)).astype(np.float32)
    dirty = padded.copy()
    dirty[:, 65:] = POISON
    a, ka = gradient(dev, padded, y, 12.0)
    b, kb = gradient(dev, dirty, y, 12.0)
    assert torch.equal(a, b) and torch.equal(ka, kb)


# ---------------------------------------------------------------------------------------------------- the descent step
def descent_state(n, seed=0):
    r = np.random.default_rng([n, seed, 13])
    y, upd, grad = (r.standard_normal((n, 2)).astype(np.float32) for _ in range(3))
    gains = (0.01 + 2.0 * r.random((n, 2))).astype(np.float32)
    upd[0] = 0.0                      # update * grad = 0: not negative, gains shrink
    grad[1] = 0.0
    upd[2, 0], grad[2, 0] = np.float32(-0.0), np.float32(1.0)
    gains[3] = np.float32(0.011)      # x 0.8 falls below min_gain: clamped
    upd[3], grad[3] = np.float32(1.0), np.float32(2.0)
    gains[4] = np.float32(0.01)
    upd[4], grad[4] = np.float32(1.0), np.float32(-2.0)   # + 0.2
    return y, upd, gains, grad


@pytest.mark.parametrize("n", [8, 63, 257, 1030])
@pytest.mark.parametrize("momentum,lr", [(0.5, 50.0), (0.8, 341.33334)])
def test_update_bit_for_bit(dev, n, momentum, lr):
    lib, _ptr, _stream = _lib()
    y, upd, gains, grad = descent_state(n)
    want = T.update(y, upd, gains, grad, momentum, lr, 0.01)
    assert want[2][3, 0] == np.float32(0.01) and want[2][0, 0] == gains[0, 0] * np.float32(0.8)
    runs = []
    for _ in range(2):
        d = [torch.from_numpy(v.copy()).to(dev) for v in (y, upd, gains, grad)]
        assert lib.mae_tsne_update(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(d[3]), n, momentum, lr, 0.01, _stream(dev)) == 0
        torch.cuda.synchronize()
        runs.append(d)
    for k, name in enumerate(("y", "update", "gains")):
        got = np_(runs[0][k])
        assert (got.view(np.uint32) == want[k].view(np.uint32)).all(), f"{name}: {int((got != want[k]).sum())} elements differ from the fp32 restatement"
        assert torch.equal(runs[0][k], runs[1][k])
    assert (np_(runs[0][3]) == grad).all()   # grad is read only


@pytest.mark.parametrize("n", [63, 1030])
def test_step_is_gradient_then_update(dev, n):
    lib, _ptr, _stream = _lib()
    P, padded = sparse_joint(n)
    y, upd, gains, _ = descent_state(n)
    grad, kl = gradient(dev, padded, y, 12.0)
    d = [torch.from_numpy(v.copy()).to(dev) for v in (y, upd, gains)]
    assert lib.mae_tsne_update(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), _ptr(grad), n, 0.5, 50.0, 0.01, _stream(dev)) == 0
    s = [torch.from_numpy(v.copy()).to(dev) for v in (y, upd, gains)]
    g2 = torch.empty_like(grad)
    kl2 = torch.full((4,), POISON, dtype=torch.float32, device=dev)
    nbytes = lib.mae_tsne_scratch_bytes(n, 1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    Pd = torch.from_numpy(padded).to(dev)
    assert lib.mae_tsne_step(_ptr(Pd), _ptr(s[0]), _ptr(s[1]), _ptr(s[2]), n, 12.0, 0.5, 50.0, 0.01, _ptr(g2), _ptr(kl2), _ptr(scratch), nbytes, _stream(dev)) == 0
    torch.cuda.synchronize()
    assert torch.equal(g2, grad) and torch.equal(kl2, kl)
    for a, b in zip(d, s):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("n,perp,word", [(7, 2.0, "n = 7"), (16385, 30.0, "n = 16385"), (100, 99.0, "perplexity"), (100, 120.0, "perplexity")])
def test_refusals_name_the_limit(dev, n, perp, word):
    lib, _, _ = _lib()
    assert lib.mae_tsne_affinities(None, n, 4, perp, None, None, None, None, None) != 0
    assert word in lib.mae_last_error().decode()
    if n != 100:
        assert lib.mae_tsne_gradient(None, None, n, 1.0, None, None, None, 0, None) != 0 and word in lib.mae_last_error().decode()
        assert lib.mae_tsne_update(None, None, None, None, n, 0.5, 50.0, 0.01, None) != 0 and word in lib.mae_last_error().decode()
        assert lib.mae_tsne_step(None, None, None, None, n, 1.0, 0.5, 50.0, 0.01, None, None, None, 0, None) != 0 and word in lib.mae_last_error().decode()


def test_short_scratch_is_refused(dev):
    lib, _ptr, _stream = _lib()
    P, padded = sparse_joint(63)
    t = torch.zeros((63, 2), dtype=torch.float32, device=dev)
    scratch = torch.empty(lib.mae_tsne_scratch_bytes(63, 1), dtype=torch.uint8, device=dev)
    g = torch.full((63, 2), POISON, dtype=torch.float32, device=dev)
    rc = lib.mae_tsne_gradient(_ptr(torch.from_numpy(padded).to(dev)), _ptr(t), 63, 1.0, _ptr(g), None, _ptr(scratch), scratch.numel() - 4, _stream(dev))
    torch.cuda.synchronize()
    assert rc != 0 and b"scratch_bytes" in lib.mae_last_error() and (np_(g) == POISON).all()
