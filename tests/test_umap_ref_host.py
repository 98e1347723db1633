"""tests/umap_ref.py and the host side of embedding.DeviceUMAP (no GPU): the curve fit pinned to the recorded constants and to
scipy.optimize.curve_fit, trustworthiness pinned to sklearn's, the properties of the reference the GPU tests lean on, DeviceUMAP's limit
errors, and the reference fit on the blob data inside the golden band of tests/golden/umap_blobs.json."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import umap_ref as R

ROOT = Path(__file__).resolve().parents[1]
A_DEFAULT, B_DEFAULT = 1.576943460, 0.895060878   # scipy 1.15.3's curve_fit at (min_dist, spread) = (0.1, 1.0), as umap-learn calls it


@pytest.fixture(scope="module")
def blob_graph():
    x, labels = R.blobs()
    return x, labels, R.graph_of(x, 15, 500)


def test_find_ab_params_gives_the_recorded_constants():
    from ssrl_vit_mae_jepa_amd.embedding import find_ab_params
    a, b = find_ab_params()
    print(f"a {a!r} b {b!r}")
    assert abs(a - A_DEFAULT) <= 1e-6 * A_DEFAULT and abs(b - B_DEFAULT) <= 1e-6 * B_DEFAULT


@pytest.mark.parametrize("min_dist,spread", [(0.1, 1.0), (0.5, 1.0), (0.0, 2.0)])
def test_find_ab_params_matches_scipy(min_dist, spread):
    curve_fit = pytest.importorskip("scipy.optimize").curve_fit
    from ssrl_vit_mae_jepa_amd.embedding import find_ab_params
    xv = np.linspace(0, spread * 3, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    (a, b), _ = curve_fit(lambda x, a, b: 1.0 / (1.0 + a * x ** (2 * b)), xv, yv)
    A, B = find_ab_params(spread, min_dist)
    print(f"({min_dist}, {spread}): scipy {a!r} {b!r}; ours {A!r} {B!r}")
    assert abs(A - a) <= 1e-6 * a and abs(B - b) <= 1e-6 * b


def test_umap_init_is_the_scaled_principal_pair_and_pca_init_is_unchanged():
    from ssrl_vit_mae_jepa_amd.embedding import pca_init, umap_init
    x, _ = R.blobs()
    u, p = umap_init(x), pca_init(x)
    assert u.dtype == np.float32 and u.shape == (600, 2) and np.abs(u).max() == np.float32(10.0)
    ratio = u.astype(np.float64) / p.astype(np.float64)
    assert np.ptp(ratio) <= 1e-5 * abs(ratio).max()                   # the same two components, another scale
    assert abs(np.std(p[:, 0].astype(np.float64)) - 1e-4) <= 1e-10     # sklearn's scale, as before


def test_trustworthiness_matches_sklearn():
    sk = pytest.importorskip("sklearn.manifold").trustworthiness
    r = np.random.default_rng(3)
    x = r.standard_normal((200, 12))
    for Z in (x[:, :2], r.standard_normal((200, 2)), x[:, :2] + 0.3 * r.standard_normal((200, 2))):
        for k in (5, 15):
            assert abs(R.trustworthiness(x, Z, k) - sk(x, Z, n_neighbors=k)) <= 1e-12


def test_smooth_sums_reach_log2_k(blob_graph):
    _, _, g = blob_graph
    ps, _ = R.smooth_sum(g["dist"], g["rho"], g["sigma"])
    free = ~g["floored"]
    assert free.any() and (g["steps"][free] < R.SEARCH_STEPS).all()
    assert (np.abs(ps[free] - np.log2(15)) < R.TOL).all()
    assert (g["rho"] == g["dist"][:, 1]).all() and (g["idx"][:, 0] == np.arange(600)).all()   # no duplicates: the point itself comes first


def test_smooth_floor_on_copies():
    """8 copies of 8 points: with k = 5 every kept distance is 0 (rho = 0, the global floor, itself 0); with k = 15 the seven other copies
    pin the sum above log2 k, the search runs out its 64 steps and the row floor holds sigma."""
    x = R.copies()
    for k in (5, 15):
        idx, dist, _ = R.knn(x, k)
        assert (np.diff(dist, axis=1) >= 0).all()
        ties = np.diff(dist, axis=1) == 0
        assert (np.diff(idx, axis=1)[ties] > 0).all()        # equal distances: index ascending
        s = R.smooth(dist)
        assert (s["steps"] == R.SEARCH_STEPS).all()
        if k == 5:
            assert (s["rho"] == 0).all() and (dist == 0).all()
        else:
            assert (s["rho"] > 0).all() and s["floored"].all()
            np.testing.assert_allclose(s["sigma"], 1e-3 * dist.mean(1), rtol=1e-15)
        m, _ = R.memberships(idx, dist, s["rho"], s["sigma"])
        own = idx == np.arange(64)[:, None]
        assert (m[own] == 0).all() and (m[~own & (dist <= s["rho"][:, None])] == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_union_is_symmetric_with_unit_nearest_weight(dtype):
    x, _ = R.blobs()
    g = R.graph_of(x, 15, 500, dtype)
    W = g["W"]
    # The nearest neighbour's membership is exactly 1 (d - rho = 0).  Its weight is (1 + m) - (1 * m) with m the reverse membership: 1 in
    # exact arithmetic, and with each operation rounded once exactly 1 where m is 0 or 1, else 1 plus the rounding of 1 + m, at most one
    # unit in the last place of a number in [1, 2].  So W lies in [0, 1 + ulp], not in [0, 1]: the arithmetic is the one DESIGN.md fixes.
    ulp = float(np.finfo(dtype).eps)
    assert W.dtype == dtype and (W == W.T).all() and W.min() >= 0 and W.max() <= 1 + ulp and (np.diag(W) == 0).all()
    rows, nearest = np.arange(600), g["idx"][:, 1]
    A = np.zeros((600, 600), dtype=dtype)
    A[rows[:, None], g["idx"]] = g["memb"].astype(dtype)
    assert (A[rows, nearest] == 1).all()
    back = A[nearest, rows]
    assert (np.abs(W[rows, nearest] - dtype(1)) <= ulp).all()
    plain = (back == 0) | (back == 1)
    assert plain.any() and (W[rows, nearest][plain] == 1).all()
    kept = W[W > 0]
    assert kept.min() >= g["wmax"] / dtype(500)
    rp, col = g["row_ptr"], g["col"]
    assert rp[0] == 0 and rp[-1] == len(col) and all((np.diff(col[rp[i]:rp[i + 1]]) > 0).all() for i in range(600))
    assert g["eps"].dtype == np.float32 and g["eps"].min() == 1.0
    pairs = set(zip(g["rows"].tolist(), col.tolist()))
    assert all((j, i) in pairs for i, j in pairs)            # both directions of every surviving edge


def test_generator_restatement():
    """fmix32 on known words (murmur3's finaliser), the index range, and no wrap of the key at the largest graph."""
    assert int(R.fmix32(0)) == 0 and int(R.fmix32(1)) == 0x514E28B7 and int(R.fmix32(0xFFFFFFFF)) == 0x81F16F39
    e = np.arange(0, 2 ** 21, 997)
    for n in (8, 600, 16384):
        k = R.negative_index(73, 499, e, 15, n)
        assert k.min() >= 0 and k.max() < n
    assert 16 * (2 * 16384 * 64 - 1) + 15 < 2 ** 32
    big = R.negative_index(5, 3, np.arange(4096), 0, 16384)
    assert abs(big.mean() / 16384 - 0.5) < 0.02              # uniform over the points
    assert (R.negative_index(5, 3, np.arange(64), 0, 600) != R.negative_index(5, 4, np.arange(64), 0, 600)).any()


def test_next_update_is_fp32():
    nxt, eps = np.array([1.0, 2.5, 3.0000002, 7.0], dtype=np.float32), np.array([1.0, 2.5, 1.1, 7.0], dtype=np.float32)
    active, out = R.next_update(nxt, eps, 3)
    assert active.tolist() == [True, True, False, False] and out.dtype == np.float32
    assert (out == np.array([2.0, 5.0, np.float32(3.0000002), 7.0], dtype=np.float32)).all()


def test_epoch_at_zero_moves_nothing(blob_graph):
    from ssrl_vit_mae_jepa_amd.embedding import umap_init
    x, _, g = blob_graph
    y = umap_init(x).astype(np.float64)
    out = R.epoch(y, g["row_ptr"], g["col"], g["eps"], g["eps"], 1.5769434, 0.8950609, 1.0, 1.0, 0, 5, 73)
    assert not out["active"].any() and (out["y"] == y).all() and (out["next"] == g["eps"]).all()
    out = R.epoch(y, g["row_ptr"], g["col"], g["eps"], g["eps"], 1.5769434, 0.8950609, 1.0, 1.0, 1, 5, 73)
    assert out["active"].sum() == (g["eps"] <= 1).sum() > 0 and (out["y"] != y).any() and np.isfinite(out["bound"]).all()


@pytest.mark.parametrize("kwargs,word", [(dict(n_neighbors=1), "n_neighbors"), (dict(n_neighbors=65), "n_neighbors"),
                                         (dict(negative_sample_rate=0), "negative_sample_rate"), (dict(negative_sample_rate=17), "negative_sample_rate"),
                                         (dict(n_epochs=0), "n_epochs"), (dict(min_dist=2.0), "min_dist")])
def test_constructor_names_the_limit(kwargs, word):
    from ssrl_vit_mae_jepa_amd.embedding import DeviceUMAP
    with pytest.raises(ValueError, match=word):
        DeviceUMAP(**kwargs)


@pytest.mark.parametrize("shape,k,word", [((7, 4), 2, "n = 7"), ((16385, 2), 15, "n = 16385"), ((20, 8193), 15, "dim = 8193"), ((15, 4), 15, "n_neighbors = 15")])
def test_prepare_names_the_limit_before_any_device_is_asked_for(shape, k, word):
    from ssrl_vit_mae_jepa_amd.embedding import DeviceUMAP
    with pytest.raises(ValueError, match=word):
        DeviceUMAP(n_neighbors=k).prepare(torch.zeros(shape), np.zeros((shape[0], 2), dtype=np.float32))   # host tensors: the limits come first
    with pytest.raises(RuntimeError, match="device tensors only"):
        DeviceUMAP().prepare(torch.zeros((20, 4)), np.zeros((20, 2), dtype=np.float32))


def test_library_refuses_by_name_without_a_device():
    from ssrl_vit_mae_jepa_amd._lib import lib
    assert lib.mae_umap_scratch_bytes(600, 32, 15) == (600 * 600 + 2 * 600) * 4
    assert lib.mae_umap_scratch_bytes(16384, 8192, 64) == (16384 * 16384 + 2 * 16384) * 4
    for bad in ((7, 4, 2), (16385, 4, 15), (100, 0, 15), (100, 8193, 15), (100, 4, 1), (100, 4, 65), (15, 4, 15)):
        assert lib.mae_umap_scratch_bytes(*bad) == -1
    for (n, dim, k), word in (((7, 4, 2), "n = 7"), ((100, 8193, 15), "dim = 8193"), ((100, 4, 65), "n_neighbors = 65"), ((15, 4, 15), "n_neighbors = 15")):
        assert lib.mae_umap_fuzzy_knn(None, n, dim, k, None, None, None, None, None, None, 0, None) != 0
        assert word in lib.mae_last_error().decode()
    for args, word in (((7, 1.0, 1.0, 1.0, 1.0, 0, 5), "n = 7"), ((100, 1.0, 1.0, 1.0, 1.0, 0, 17), "negative_sample_rate = 17"),
                       ((100, 1.0, 1.0, 1.0, 1.0, -1, 5), "t = -1"), ((100, 0.0, 1.0, 1.0, 1.0, 0, 5), "curve"), ((100, 1.0, 1.0, 1.0, 1.0, 0, 5), "null")):
        assert lib.mae_umap_epoch(None, None, None, None, None, None, *args, 73, None) != 0
        assert word in lib.mae_last_error().decode()


def test_reference_fit_on_the_blobs_is_inside_the_golden_band(blob_graph):
    from ssrl_vit_mae_jepa_amd.embedding import find_ab_params, umap_init
    x, labels, g = blob_graph
    golden = json.loads((ROOT / "tests" / "golden" / "umap_blobs.json").read_text())
    a, b = (float(np.float32(v)) for v in find_ab_params())
    assert abs(a - golden["a"]) <= 1e-6 and abs(b - golden["b"]) <= 1e-6
    Z = R.fit(x, umap_init(x), a, b, seed=golden["seeds"][0], graph=g)["Z"]
    trust, acc = R.trustworthiness(x, Z, 15), R.loo_1nn_accuracy(Z, labels)
    lo, hi = min(golden["trustworthiness"]), max(golden["trustworthiness"])
    print(f"trustworthiness {trust:.6f} (golden {lo:.6f} .. {hi:.6f}, limit {golden['limit']:.6f}); accuracy {acc} (limit {golden['accuracy_limit']}); "
          f"max |y| {np.abs(Z).max():.2f}; sequential {golden['sequential']}")
    assert np.isfinite(Z).all()
    assert golden["limit"] == lo - (hi - lo) and golden["accuracy_limit"] == min(golden["accuracy"])
    assert trust >= golden["limit"] and acc >= golden["accuracy_limit"]
