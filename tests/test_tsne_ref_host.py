"""tests/tsne_ref.py pinned to sklearn's own internals on float32-representable distances (no GPU): the conditional P of
sklearn.manifold._utils._binary_search_perplexity, the gradient and KL of sklearn.manifold._t_sne._kl_divergence, the descent step of
_t_sne._gradient_descent, and the properties of the reference the GPU tests lean on."""
import numpy as np
import pytest
from scipy.spatial.distance import squareform

from tests import tsne_ref as T

SHAPES = [(600, 30.0), (240, 50.0), (120, 5.0)]


@pytest.fixture(scope="module")
def cases():
    out = {}
    for n, perp in SHAPES:
        x = T.gen_features(n, 16, seed=n)
        D = T.sqdist(x).astype(np.float32)          # what sklearn's search takes; the reference gets the same values
        out[(n, perp)] = (D, T.search(D.astype(np.float64), perp))
    return out


@pytest.mark.parametrize("n,perp", SHAPES)
def test_conditional_p_matches_sklearn_on_every_row(cases, n, perp):
    from sklearn.manifold._utils import _binary_search_perplexity
    D, ref = cases[(n, perp)]
    sk = np.asarray(_binary_search_perplexity(D, perp, 0), dtype=np.float64)   # before sklearn's machine-epsilon floor
    assert (ref["steps"] < T.MAX_STEPS).all()
    err = np.abs(ref["p_cond"] - sk).max(1) / sk.max(1)
    print(f"n {n} perplexity {perp}: worst row {err.max():.2e}")
    assert (err <= 1e-12).all(), f"rows {np.nonzero(err > 1e-12)[0][:8]} differ: worst {err.max():.3e}"
    np.testing.assert_allclose(ref["p_cond"].sum(1), 1.0, rtol=0, atol=1e-13)
    assert (np.diag(ref["p_cond"]) == 0).all()
    np.testing.assert_allclose(T.entropy(D, ref["beta"]), np.log(perp), rtol=0, atol=T.TOL)


@pytest.mark.parametrize("n,perp", SHAPES)
@pytest.mark.parametrize("scale", [1e-4, 1.0, 50.0])
def test_gradient_and_kl_match_sklearn(cases, n, perp, scale):
    from sklearn.manifold._t_sne import _kl_divergence
    _, ref = cases[(n, perp)]
    P = T.joint(ref["p_cond"])
    y = scale * np.random.default_rng([n, 3]).standard_normal((n, 2))
    kl, grad = _kl_divergence(y.ravel().copy(), squareform(P, checks=False), 1.0, n, 2)
    mine = T.gradient(P, y, 1.0)
    # sklearn's log Z comes multiplied by the sum of P, the reference's by exactly 1
    assert abs(mine["kl"] - np.log(mine["Z"]) * (1.0 - P.sum()) - kl) <= 1e-12 * max(1.0, abs(kl))
    g = grad.reshape(n, 2)
    assert np.abs(mine["grad"] - g).max() <= 1e-12 * np.abs(g).max()


def test_joint_is_symmetric_and_sums_to_one(cases):
    _, ref = cases[(240, 50.0)]
    P = T.joint(ref["p_cond"])
    assert (P == P.T).all() and (np.diag(P) == 0).all() and abs(P.sum() - 1.0) < 1e-13


def test_update_matches_sklearn_gradient_descent():
    """One iteration of sklearn's _gradient_descent on a linear objective gives the reference's step."""
    from sklearn.manifold._t_sne import _gradient_descent
    r = np.random.default_rng(4)
    y0, g = r.standard_normal((50, 2)), r.standard_normal((50, 2))

    def objective(p, *a, **k):
        return 0.0, g.ravel().copy()

    for momentum in (0.5, 0.8):
        p, _, _ = _gradient_descent(objective, y0.ravel().copy(), 0, 1, n_iter_check=1000, momentum=momentum, learning_rate=50.0, min_gain=0.01,
                                    min_grad_norm=0.0)
        y1, u1, g1 = T.update(y0, np.zeros_like(y0), np.ones_like(y0), g, momentum, 50.0, 0.01)
        np.testing.assert_allclose(p.reshape(50, 2), y1, rtol=1e-15)
        assert (g1 == 0.8).all()          # update = 0: the product is never negative


def test_update_in_float32_rounds_every_operation_once():
    r = np.random.default_rng(5)
    y, u, ga, g = (r.standard_normal((37, 2)).astype(np.float32) for _ in range(4))
    ga = np.abs(ga) + np.float32(0.01)
    y1, u1, g1 = T.update(y, u, ga, g, 0.8, 50.0, 0.01)
    assert y1.dtype == u1.dtype == g1.dtype == np.float32
    inc = (u.astype(np.float64) * g) < 0
    want_g = np.maximum(np.where(inc, (ga.astype(np.float64) + np.float32(0.2)).astype(np.float32), (ga.astype(np.float64) * np.float32(0.8)).astype(np.float32)),
                        np.float32(0.01))
    assert (g1 == want_g).all()
    gg = (g.astype(np.float64) * g1).astype(np.float32)
    a, b = (np.float32(0.8) * u.astype(np.float64)).astype(np.float32), (np.float32(50.0) * gg.astype(np.float64)).astype(np.float32)
    assert (u1 == (a.astype(np.float64) - b).astype(np.float32)).all()


def test_search_restated_with_float32_beta_still_converges(cases):
    D, ref = cases[(120, 5.0)]
    r32 = T.search(D.astype(np.float64), 5.0, beta_dtype=np.float32)
    assert (r32["steps"] < T.MAX_STEPS).all()
    assert np.abs(r32["H"] - np.log(5.0)).max() <= T.TOL


def test_shift_leaves_p_unchanged_and_saves_a_far_row():
    x = T.gen_features(65, 4, case="outlier")
    D = T.sqdist(x)
    ref = T.search(D, 30.0)
    assert np.isfinite(ref["p_cond"]).all()
    np.testing.assert_allclose(ref["p_cond"].sum(1), 1.0, atol=1e-13)   # unshifted, e^(-beta d) of row 2 underflows to a zero sum at beta = 1
    assert np.exp(-np.delete(D[2], 2)).sum() == 0.0


def test_bounds_tell_a_two_ulp_error_from_a_correct_result():
    """The gradient bound is a small multiple of fp32 resolution: a value rounded to fp32 passes, one moved by 1e-5 relative does not."""
    x, _ = T.blobs(3, 20, 8, seed=1)
    P = T.affinities(x, 10.0)
    y = np.random.default_rng(2).standard_normal((60, 2))
    ref = T.gradient(P, y, 12.0)
    b = T.gradient_bound(ref, 12.0, 60)
    assert (np.abs(ref["grad"].astype(np.float32).astype(np.float64) - ref["grad"]) <= b).all()
    assert (np.abs(ref["grad"] * 1e-5) > b).mean() > 0.9


def test_blobs_are_the_issue_data():
    x, labels = T.blobs()
    assert x.shape == (600, 32) and x.dtype == np.float32 and (np.bincount(labels) == 100).all()
    assert not (labels[:-1] <= labels[1:]).all()            # shuffled
    assert T.loo_1nn_accuracy(x, labels) == 1.0             # separable in feature space
