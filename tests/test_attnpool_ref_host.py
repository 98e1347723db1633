"""The attentive probe's float64 reference (tests/attnpool_ref.py) checked on the CPU: the folded form against the unfolded definition
and its autograd, the definition's gradients against central differences, sum_t ds = 0, and the checker itself: the bounds pass a
plain fp32 evaluation and flag the two faults a kernel of this kind is most likely to have."""
import numpy as np
import pytest

from tests import attnpool_ref as R

SHAPES = [(5, 37, 48, 6, 10), (2, 9, 16, 1, 3), (3, 5, 20, 5, 4)]


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300))


def probe_inputs(B, T, D, H, C, seed=0):
    r = np.random.default_rng([B, T, D, H, C, seed])
    x = 1.3 * r.standard_normal((B, T, D)) + 3.0 * r.standard_normal(D)
    return dict(x=x, q=0.5 * r.standard_normal(D), wk=0.3 * r.standard_normal((D, D)), wv=0.3 * r.standard_normal((D, D)),
                w=0.3 * r.standard_normal((C, D)), b=0.1 * r.standard_normal(C), labels=r.integers(0, C, B))


@pytest.mark.parametrize("B,T,D,H,C", SHAPES)
def test_folded_form_equals_the_definition(B, T, D, H, C):
    i = probe_inputs(B, T, D, H, C)
    ref = R.definition(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H)
    got = R.folded(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H)
    for k in ("p", "dq", "dwk", "dwv", "dw", "db"):
        assert rel(got[k], ref[k]) <= 1e-12, (k, rel(got[k], ref[k]))
    assert abs(got["loss"] - float(ref["loss"])) <= 1e-12 * abs(float(ref["loss"]))
    assert np.abs(got["ds"].sum(1)).max() <= 1e-12 * np.abs(got["ds"]).sum(1).max()          # sum_t ds = 0
    assert rel(got["a"], ref["a"]) <= 1e-12


def test_evaluation_form_uses_the_given_statistics():
    B, T, D, H, C = SHAPES[0]
    i = probe_inputs(B, T, D, H, C)
    r = np.random.default_rng(5)
    stats = (r.standard_normal(D), 0.5 + r.random(D))
    ref = R.definition(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H, stats=stats)
    got = R.folded(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H, stats=stats)
    assert rel(got["logits"], ref["logits"]) <= 1e-12
    batch = R.definition(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H)
    assert rel(batch["logits"], ref["logits"]) > 1e-3                                         # the statistics matter


def test_reference_gradients_agree_with_central_differences():
    B, T, D, H, C = 3, 7, 12, 3, 4
    i = probe_inputs(B, T, D, H, C, seed=2)
    ref = R.definition(i["x"], i["q"], i["wk"], i["wv"], i["w"], i["b"], i["labels"], H)
    r = np.random.default_rng(9)
    h = 1e-6
    for name, key in (("q", "dq"), ("wk", "dwk"), ("wv", "dwv"), ("w", "dw"), ("b", "db")):
        for _ in range(6):
            idx = tuple(int(r.integers(0, n)) for n in i[name].shape)
            lo, hi = dict(i), dict(i)
            lo[name], hi[name] = i[name].copy(), i[name].copy()
            lo[name][idx] -= h
            hi[name][idx] += h
            fl = float(R.definition(lo["x"], lo["q"], lo["wk"], lo["wv"], lo["w"], lo["b"], i["labels"], H)["loss"])
            fh = float(R.definition(hi["x"], hi["q"], hi["wk"], hi["wv"], hi["w"], hi["b"], i["labels"], H)["loss"])
            fd = (fh - fl) / (2 * h)
            assert abs(fd - ref[key][idx]) <= 1e-6 * max(abs(ref[key][idx]), np.abs(ref[key]).max() * 1e-3), (name, idx, fd, ref[key][idx])


def test_geometry():
    assert R.geometry(384, 6, 144, 2000) == dict(nv=2, hg=2, hpw=3, ts=2, kd=14, nch_fwd=18, nch_bwd=36, ipb=4, grid=500,
                                                 bwd_scratch_bytes=500 * 6 * 384 * 4, wv_slices=8)
    g = R.geometry(1024, 16, 257, 3)
    assert (g["nv"], g["hg"], g["hpw"], g["ts"], g["ipb"], g["grid"]) == (4, 4, 4, 1, 1, 3)
    g = R.geometry(64, 4, 2, R.MANY_IMAGES)
    assert g["ipb"] == 3 and g["grid"] == 343 and g["grid"] < R.MANY_IMAGES
    cases = R.kernel_cases()
    assert {c[1] for c in cases if c[2:] == (384, 6)} == set(R.T_LIST)
    assert {c[2:] for c in cases if c[1] == 145} == set(R.DH_LIST)
    assert {c[0] for c in cases} >= {1, 3, R.MANY_IMAGES}


# ------------------------------------------------------------------------------------------------ the checker
def f32_pieces(c, H):
    """The folded pieces evaluated in fp32 by numpy (its own summation order: the bounds do not depend on one)."""
    f = np.float32
    x, mean, rstd = c["x"], c["mean"], c["rstd"]
    D = x.shape[-1]
    hd = D // H
    uq = (rstd * (f(hd ** -0.5) * np.einsum("hj,hjd->hd", c["q"].reshape(H, hd), c["wk"].reshape(H, hd, D)))).astype(f)
    cc = x - mean
    s = np.einsum("btd,hd->bth", cc, uq).astype(f)
    m = s.max(1, keepdims=True)
    w = np.exp(s - m).astype(f)
    L = w.sum(1, keepdims=True, dtype=f)
    ybar = (np.einsum("bth,btd->bhd", w, cc).astype(f) / L.transpose(0, 2, 1)).astype(f)
    lse = (m + np.log(L))[:, 0].astype(f)
    return uq, ybar, lse


@pytest.mark.parametrize("B,T,D,H", [(3, 145, 384, 6), (2, 65, 64, 4), (1, 257, 1024, 16)])
def test_bounds_pass_an_fp32_evaluation_and_flag_a_wrong_ybar(B, T, D, H):
    c = R.gen_case(B, T, D, H)
    uq, ybar, lse = f32_pieces(c, H)
    ratio, _ = R.worst(uq, R.fold(c["q"], c["wk"], c["rstd"], H), R.fold_bound(c["q"], c["wk"], c["rstd"], H))
    assert ratio <= 1.0, ratio
    ref = R.pool_fwd(c["x"], c["mean"], uq)
    b = R.pool_fwd_bounds(ref, uq, True, H)
    ry, _ = R.worst(ybar, ref["ybar"], b["ybar"])
    rl, _ = R.worst(lse, ref["lse"], b["lse"])
    assert ry <= 1.0 and rl <= 1.0, (ry, rl)
    if D == 1024:
        return   # 1024 columns of score error leave the bound of every element above 2^-12 of it (0.89 at best): only the pass is checked
    # one element off by 2^-12 relative: the element where that is largest against its bound
    i = int(np.argmax(np.abs(ref["ybar"]) / b["ybar"]))
    bad = ybar.copy().reshape(-1)
    bad[i] = np.float32(ref["ybar"].reshape(-1)[i] * (1.0 + 2.0 ** -12))
    ratio, at = R.worst(bad.reshape(ybar.shape), ref["ybar"], b["ybar"])
    assert ratio > 1.0 and at == i, (ratio, at, i)


@pytest.mark.parametrize("B,T,D,H", [(3, 145, 384, 6), (4, 9, 64, 4)])
def test_bounds_flag_a_duq_that_misses_one_image(B, T, D, H):
    c = R.gen_case(B, T, D, H)
    uq, ybar, lse = f32_pieces(c, H)
    g = R.project_bwd(c["dp"], ybar, c["rstd"], c["wv"], H)["g"].astype(np.float32)
    ref = R.pool_bwd(c["x"], c["mean"], uq, lse, ybar, g)
    bound = R.pool_bwd_bounds(ref, uq, lse, ybar, g, True, H)
    good = np.einsum("bth,btd->hd", ref["ds"].astype(np.float32), ref["c"].astype(np.float32)).astype(np.float32)
    assert R.worst(good, ref["duq"], bound)[0] <= 1.0
    short = R.pool_bwd(c["x"][:-1], c["mean"], uq, lse[:-1], ybar[:-1], g[:-1])["duq"]
    assert R.worst(short.astype(np.float32), ref["duq"], bound)[0] > 1.0
