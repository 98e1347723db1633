"""The LayerNorm reference (tests/ln_ref.py) checked on the host: the float64 formulas against torch, the restated dispatcher and
launch geometry, the case table against the list of edges it has to reach, the bounds against an fp32 emulation of both kernels
in the kernels' own order (lane-group partial sums, butterfly shuffles, a serial walk over the trips of a lane group, the LDS
combine, the two-level second stage), and the proof that the checks tell wrong kernels apart: every mutant of the emulation fails
in a case named here.  The data is the data of the GPU tests, so everything those impose is first shown to hold for the reference
and the emulation alone."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import ln_ref as R

F = np.float32
CASES = R.cases()
BY_ID = {c.id: c for c in CASES}


# ------------------------------------------------------------------------------------------------ the emulation
def _fma(a, b, c):
    """fl(a b + c) in one rounding: the product of two fp32 numbers is exact in double."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def _lanes(a, geo):
    """(n, dim) -> (n, NV, lpr, 4): vector i of lane li is float4 column li + lpr i; columns past dim hold zeros."""
    p = np.zeros((a.shape[0], geo.nv * geo.lpr * 4), F)
    p[:, :geo.dim] = a
    return p.reshape(a.shape[0], geo.nv, geo.lpr, 4)


def _flat(a, geo):
    return a.reshape(a.shape[0], -1)[:, :geo.dim]


def _group_sum(s, lpr):
    """__shfl_xor butterfly over the lpr lanes of a group: (n, lpr) -> (n,)"""
    idx, o = np.arange(lpr), lpr // 2
    while o:
        s = s + s[:, idx ^ o]
        o >>= 1
    return s[:, 0]


def _sum4(t):
    return ((t[..., 0] + t[..., 1]) + t[..., 2]) + t[..., 3]


def _dot4(a, b, fma):
    if fma:
        acc = a[..., 0] * b[..., 0]
        for k in (1, 2, 3):
            acc = _fma(a[..., k], b[..., k], acc)
        return acc
    return ((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]) + a[..., 3] * b[..., 3]


def _mask(geo):
    """(NV, lpr, 1): float4 column inside the row"""
    c4 = np.arange(geo.nv)[:, None] * geo.lpr + np.arange(geo.lpr)[None, :]
    return (c4 < geo.dim // 4)[:, :, None]


def _trip(geo, rows, grid):
    return (np.arange(rows) // geo.rpw) // (grid * 4)


def emulate_fwd(c, d, fma=False, mutant=None):
    """layernorm_fwd_kernel in fp32, operation by operation.  -> (out dict as check_fwd takes it, x_out before the launch)."""
    geo, rows, dim = c.geo, c.rows, c.dim
    src = R._src(rows, d["row_map"])
    v = d["x"][src]
    init = xo = None
    if c.add:
        v = v + d["branch"][src]
        init = np.full((c.src_rows, dim), np.nan, F)
        xo = init.copy()
        xo[src] = v
    ln, m = _lanes(v, geo), _mask(geo)
    s = np.zeros((rows, geo.lpr), F)
    for i in range(geo.nv):
        s = s + _sum4(ln[:, i])
    inv_d = F(1) / F(geo.nv * geo.lpr * 4 if mutant == "inv_d_padded" else dim)
    mean = _group_sum(s, geo.lpr) * inv_d
    tot = _group_sum(s, geo.lpr)[:, None, None, None]
    # fused: v - sum * inv_d contracted into one fma (the mean that is stored stays the rounded product)
    dl = np.where(m, _fma(-tot, inv_d, ln) if fma else ln - mean[:, None, None, None], F(0))
    sq = np.zeros((rows, geo.lpr), F)
    for i in range(geo.nv):
        t = ln[:, i] if mutant == "var_ex2" else dl[:, i]
        sq = sq + _dot4(t, t, fma)
    var = _group_sum(sq, geo.lpr) * inv_d
    if mutant == "var_ex2":
        var = var - mean * mean
    eps = F(1e-5) if mutant == "eps_1e-5" else F(R.EPS)
    arg = _fma(_group_sum(sq, geo.lpr), inv_d, eps) if fma else var + eps
    with np.errstate(invalid="ignore"):
        rstd = (1.0 / np.sqrt(arg.astype(np.float64))).astype(F)          # a correctly rounded rsqrtf
    gl, bl = _lanes(d["gamma"][None], geo), _lanes(d["beta"][None], geo)
    t = dl * rstd[:, None, None, None]
    y = _flat(_fma(t, gl, bl) if fma else t * gl + bl, geo)
    assert y.dtype == F and mean.dtype == F and rstd.dtype == F
    if c.dtype == "bf16":
        y = R.to_bf16(y)
    dead = np.zeros(rows, bool)
    if mutant == "last_row_skipped":
        dead[rows - 1] = True
    if mutant == "trip_repeats":
        dead = _trip(geo, rows, geo.fwd_grid) > 0
    y, mean, rstd = y.copy(), mean.copy(), rstd.copy()
    y[dead], mean[dead], rstd[dead] = np.nan, np.nan, np.nan
    if c.add:
        xo[src[dead]] = np.nan
    return dict(y=y, mean=mean, rstd=rstd, x_out=xo), init


def emulate_bwd(c, d, mean, rstd, fma=False, mutant=None):
    """layernorm_bwd_kernel + sum_partials_kernel in fp32.  -> (out dict as check_bwd takes it, dx before the launch)."""
    geo, rows, dim = c.geo, c.rows, c.dim
    src = R._src(rows, d["row_map"])
    dy = d["dy"][src % rows] if mutant == "dy_through_map" else d["dy"]
    xl, dyl, gl, m = _lanes(d["x"][src], geo), _lanes(dy, geo), _lanes(d["gamma"][None], geo), _mask(geo)
    mu, rs = mean[:, None, None, None], rstd[:, None, None, None]
    xh = np.where(m, (xl - mu) * rs, F(0))
    g = dyl * gl
    s1, s2 = np.zeros((rows, geo.lpr), F), np.zeros((rows, geo.lpr), F)
    for i in range(geo.nv):
        s1 = s1 + _sum4(dyl[:, i] if mutant == "s1_of_dy" else g[:, i])
        s2 = s2 + _dot4(g[:, i], xh[:, i], fma)
    inv_d = F(1) / F(dim)
    s1 = (_group_sum(s1, geo.lpr) * inv_d)[:, None, None, None]
    s2 = (_group_sum(s2, geo.lpr) * inv_d)[:, None, None, None]
    dx = _flat((_fma(-xh, s2, g - s1) if fma else (g - s1) - xh * s2) * rs, geo)
    init = d["res"].copy() if c.accumulate else np.full((c.src_rows, dim), np.nan, F)
    if c.accumulate and mutant != "accumulate_ignored":
        dx = dx + d["res"][src]
    assert dx.dtype == F
    trip = _trip(geo, rows, geo.bwd_grid)
    done = np.ones(rows, bool)
    if mutant == "last_row_skipped":
        done[rows - 1] = False
    if mutant == "trip_repeats":
        done = trip == 0
    out_dx = init.copy()
    out_dx[src[done]] = dx[done]
    out_copy = None
    if c.copy:
        out_copy = np.full((c.src_rows, dim), np.nan, F)
        out_copy[(np.arange(rows) if mutant == "dx_copy_compact" else src)[done]] = (R.to_bf16(dx) if c.dtype == "bf16" else dx)[done]
    # column partials: slot (trip, lane group) of every row; a lane group adds its rows trip by trip
    ng, T, W = geo.bwd_grid * 4 * geo.rpw, geo.bwd_trips, geo.nv * geo.lpr * 4
    slot_row = np.full(T * ng, -1, np.int64)
    slot_row[np.arange(rows)] = np.arange(rows)          # slot = trip * ng + (row mod ng): row order is slot order
    if mutant == "dead_group_adds":                       # lane groups past the last row of its wave add the clamped row
        slot_row[rows:R.cdiv(rows, geo.rpw) * geo.rpw] = rows - 1
    if mutant == "last_row_skipped":
        slot_row[rows - 1] = -1
    if mutant == "trip_repeats":
        active = np.arange(T * ng) // geo.rpw * geo.rpw < rows          # the wave's loop variable still advances
        slot_row = np.where(active, np.tile(slot_row[:ng], T), -1)
    dg, db = np.zeros((ng, W), F), np.zeros((ng, W), F)
    dyf, xhf = dyl.reshape(rows, W), xh.reshape(rows, W)
    for t in range(T):
        sr = slot_row[t * ng:(t + 1) * ng]
        live = (sr >= 0)[:, None]
        a, b = np.where(live, dyf[sr], F(0)), np.where(live, xhf[sr], F(0))
        dg = _fma(a, b, dg) if fma else dg + a * b
        db = db + a
    outs = []
    for part in (dg, db):
        red = part.reshape(geo.bwd_grid, 4 * geo.rpw, W)
        v = np.zeros((geo.bwd_grid, W), F)
        for gi in range(4 * geo.rpw):                     # the block's serial sum over LDS
            v = v + red[:, gi]
        G = geo.bwd_grid
        S = G // R.SP_LANES if mutant == "second_stage_drops_tail" else R.cdiv(G, R.SP_LANES)
        p = np.zeros((max(S, 1) * R.SP_LANES, W), F)
        n = min(G, S * R.SP_LANES)
        p[:n] = v[:n]
        acc = np.zeros((R.SP_LANES, W), F)
        for srow in p.reshape(-1, R.SP_LANES, W):         # row lane rl adds partial rows rl, rl + 32, ..
            acc = acc + srow
        o = np.zeros(W, F)
        for j in range(R.SP_LANES):
            o = o + acc[j]
        assert o.dtype == F
        outs.append(o[:dim])
    return dict(dx=out_dx, dx_copy=out_copy, dgamma=outs[0], dbeta=outs[1]), init


def run_case(c, fma=False, mutant=None, exact=False):
    """-> (ratios of every output, failures) of the emulation on case c, through the checks the GPU test applies."""
    if exact:
        d = R.gen_exact(c)
        mean, rstd = d["mean"], d["rstd"]
        d["kinds"] = np.zeros(c.rows, np.int64)
        out, _ = emulate_fwd(c, d, fma, mutant)
        fails = R.check_exact_fwd(c, d, out)
        ratios = {}
    else:
        d = R.gen_case(c)
        mean, rstd = R.bwd_stats(c, d)
        out, init = emulate_fwd(c, d, fma, mutant)
        ratios, fails = R.check_fwd(c, d, out, init)
    out, init = emulate_bwd(c, d, mean, rstd, fma, mutant)
    r2, f2 = R.check_bwd(c, d, mean, rstd, out, init, exact)
    ratios.update(r2)
    return ratios, fails + f2


# ------------------------------------------------------------------------------------------------ formulas, dispatcher, table
def test_reference_equals_torch_layer_norm_in_float64():
    g = torch.Generator().manual_seed(3)
    rows, n, dim = 9, 14, 68
    x = torch.randn(n, dim, dtype=torch.float64, generator=g).float()
    gamma, beta = torch.randn(dim, generator=g), torch.randn(dim, generator=g)
    rmap = torch.randperm(n, generator=g)[:rows]
    dy, res = torch.randn(rows, dim, generator=g), torch.randn(n, dim, generator=g)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    y = TF.layer_norm(xr[rmap], (dim,), gr, br, R.f32(R.EPS))
    y.backward(dy.double())
    ref = R.fwd_ref(x.numpy(), gamma.numpy(), beta.numpy(), rows, rmap.numpy())
    np.testing.assert_allclose(ref["y"], y.detach().numpy(), rtol=1e-12, atol=1e-13)
    b = R.bwd_ref(dy.numpy(), x.numpy(), gamma.numpy(), ref["mean"], ref["rstd"], rows, rmap.numpy(), 1, res.numpy())
    np.testing.assert_allclose(b["dx"], (xr.grad + res.double())[rmap].numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(b["dgamma"], gr.grad.numpy(), rtol=1e-11, atol=1e-12)
    np.testing.assert_allclose(b["dbeta"], br.grad.numpy(), rtol=1e-12, atol=1e-12)
    br16 = R.to_bf16(torch.randn(n, dim, generator=g).numpy())
    a = R.fwd_ref(x.numpy(), gamma.numpy(), beta.numpy(), rows, rmap.numpy(), br16)
    assert np.array_equal(a["x_out"], (x + torch.from_numpy(br16))[rmap].numpy())   # fl32(x + branch) is the fp32 sum


def test_dispatcher_selects_exactly_the_eight_pairs():
    seen = {}
    for dim in range(4, 1025, 4):
        g = R.geometry(1, dim)
        assert g.nv <= 4 and g.lpr * g.nv * 4 >= dim
        seen.setdefault((g.lpr, g.nv), []).append(dim)
    assert {k: (v[0], v[-1]) for k, v in seen.items()} == {(lpr, nv): (lo, hi) for lpr, nv, lo, hi in R.PAIRS}
    for dims in seen.values():
        assert dims == list(range(dims[0], dims[-1] + 1, 4))          # each pair owns one interval of dims
    assert not set(R.UNREACHABLE) & set(seen) and len(seen) + len(R.UNREACHABLE) == 12


def test_geometry_counts():
    g = R.geometry(70001, 192)
    assert (g.lpr, g.nv, g.rpw, g.fwd_grid, g.bwd_grid, g.fwd_trips, g.bwd_trips) == (16, 3, 4, 4376, 1024, 1, 5)
    assert (g.lds_floats, g.sp_blocks, g.sp_strided) == (8 * 4 * 192, 12, 32)
    for rows, dim, lpr in R.FWD_WRAPS[0][:2] + (64,), R.FWD_WRAPS[1][:2] + (32,), R.FWD_WRAPS[2][:2] + (16,):
        g = R.geometry(rows, dim)
        assert (g.lpr, g.fwd_grid, g.fwd_trips) == (lpr, 8192, 2)
        assert R.geometry(8192 * 4 * g.rpw, dim).fwd_trips == 1
    for rows, dim, lpr in R.BWD_WRAPS[0][:2] + (64,), R.BWD_WRAPS[1][:2] + (32,), R.BWD_WRAPS[2][:2] + (16,):
        g = R.geometry(rows, dim)
        assert (g.lpr, g.bwd_grid, g.bwd_trips, g.fwd_trips) == (lpr, 1024, 2, 1)
    assert R.lds_index(g, 3, g.rpw - 1, 1, g.dim - 1) == g.lds_floats - 1 and R.lds_index(g, 0, 1, 0, 0) == 2 * g.dim
    g = R.geometry(133, 64)
    assert (g.bwd_grid, g.sp_strided) == (9, 1) and "block 8 wave 1 lane group 0" in R.locate(g, 132, 5, True)
    assert "trip 1 of 2" in R.locate(R.geometry(4097, 512), 4096, 0, True)


def test_case_table_leaves_no_gap():
    assert R.coverage_gaps(CASES) == []
    assert len({c.id for c in CASES}) == len(CASES)
    labels = {c.label for c in CASES}
    assert len(labels) == 2 * 8 * 2                                       # dtype x pair x ADD
    assert max(c.src_rows * c.dim for c in CASES) * 4 < 30e6              # no tensor above 30 MB
    # the function does see gaps
    assert any("forward wrap at 16" in s for s in R.coverage_gaps([c for c in CASES if not (c.kind == "fwd_wrap" and c.dim == 8)]))
    assert any("dim 388" in s for s in R.coverage_gaps([c for c in CASES if c.dim != 388]))
    assert any("33 blocks" in s for s in R.coverage_gaps([c for c in CASES if c.geo.bwd_grid != 33]))
    assert any("accumulate 0" in s for s in R.coverage_gaps([c for c in CASES if not (c.map and c.copy and c.accumulate == 0)]))


@pytest.mark.parametrize("dim", sorted({c.dim for c in CASES}))
def test_generated_data_is_what_the_gpu_tests_need(dim):
    """The row kinds, nothing near the denormals, the constant rows' float64 mean exact, the exactness data below 2^24."""
    tiny = float(np.finfo(F).tiny)
    for c in (c for c in CASES if c.dim == dim and c.dtype == "bf16" and c.kind == "table"):
        d = R.gen_case(c)
        ref = R.fwd_ref(d["x"], d["gamma"], d["beta"], c.rows, d["row_map"], d["branch"])
        k = d["kinds"]
        if c.rows > 3:
            assert (k == 2).sum() == 1 and (k == 1).sum() >= 1 and (k == 0).sum() >= 1 and k[-1] == 0
        assert d["const"] == (3.0 if R.is_pow2(dim) else 0.0)
        if c.rows > 4:
            assert np.all(ref["mean"][k == 3] == 3.0) and np.all(ref["var"][k == 3] == 0.0) and k[-1] == 0
        assert np.all(ref["var"][k == 2] == 0.0) and np.all(ref["mean"][k == 2] == d["const"])
        assert np.all(np.abs(ref["mean"][k == 1]) > 1e3 * np.sqrt(ref["var"][k == 1]))   # mean large against the spread
        mean, rstd = R.bwd_stats(c, d)
        b = R.bwd_ref(d["dy"], d["x"], d["gamma"], mean, rstd, c.rows, d["row_map"], c.accumulate, d["res"])
        for name, a in (("x", d["x"]), ("dy", d["dy"]), ("gamma", d["gamma"]), ("beta", d["beta"]), ("d^2", ref["d"] ** 2), ("y", ref["y"]),
                        ("g xh", b["g"] * b["xh"]), ("dy xh", d["dy"] * b["xh"]), ("dx", b["dx"]), ("dgamma", b["dgamma"]), ("dbeta", b["dbeta"])):
            a = np.abs(np.asarray(a, np.float64))
            assert a[a != 0].min() > 64 * tiny and np.isfinite(a).all(), (c.id, name)
        if c.dtype == "bf16":
            assert np.array_equal(R.to_bf16(d["dy"]), d["dy"]) and (d["branch"] is None or np.array_equal(R.to_bf16(d["branch"]), d["branch"]))
        e = R.gen_exact(c)
        assert np.abs(e["dy"]).max() * np.abs(e["x"]).max() * 2.0 * max(c.rows, c.dim) * np.abs(e["gamma"]).max() < 2 ** 24


# ------------------------------------------------------------------------------------------------ the bounds hold, the mutants fall
@pytest.mark.parametrize("fma", [False, True], ids=["separate", "fused"])
def test_faithful_emulation_stays_inside_every_bound(fma):
    worst = {}
    for c in CASES:
        if fma and c.kind != "table" and c.dtype == "bf16":
            continue                                             # the wraps once per variant and once per dtype are enough
        ratios, fails = run_case(c, fma)
        assert not fails, (c.id, fails)
        for k, v in ratios.items():
            key = (c.label if k in ("y", "mean", "rstd") else c.label.replace(f"ADD {int(c.add)}, ", ""), k)
            worst[key] = max(worst.get(key, 0.0), v)
    for (label, k), v in sorted(worst.items()):
        print(f"{label:34s} {k:8s} {v:.3f}")
    assert max(worst.values()) <= 1.0


def test_faithful_emulation_is_exact_on_the_exactness_data():
    for c in CASES:
        if c.dtype == "bf16" and c.rows != 1001:
            continue                                             # every fp32 case, and the bf16 rounding of dx_copy at 1001 rows
        ratios, fails = run_case(c, fma=True, exact=True)
        assert not fails, (c.id, fails)


# mutant -> (the case that catches it, the output or check that fails there)
MUTANTS = {
    "var_ex2": ("fp32-1001x192-add-map-acc0-copy", "rstd"),                     # variance as E[x^2] - mean^2: the large-mean rows
    "eps_1e-5": ("fp32-5x256-add-map-acc1-copy", "rstd"),                        # the constant row: rstd = rsqrt(eps)
    "inv_d_padded": ("fp32-17x4-add-map-acc1-copy", "mean"),                    # 1 / 64 for a row of 4
    "dead_group_adds": ("fp32-17x132-add-map-acc1-copy", "dbeta"),              # 4R + 1 rows: three lane groups of the last wave have no row
    "last_row_skipped": ("fp32-17x192-add-map-acc1-copy", "y"),
    "dy_through_map": ("bf16-16x64-ln-map-acc0-copy", "dx"),
    "dx_copy_compact": ("bf16-16x64-ln-map-acc0-copy", "dx_copy"),              # the engine's form
    "accumulate_ignored": ("fp32-130x1024-add-all-acc1-nocopy", "dx"),
    "s1_of_dy": ("fp32-1x516-ln-all-acc1-copy", "dx"),
    "second_stage_drops_tail": ("fp32-130x388-ln-all-acc1-nocopy", "dgamma"),   # 33 blocks: the 33rd is dropped
    "trip_repeats": ("fp32-4097x512-ln-map-acc0-copy", "dx"),                   # the backward's second trip
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_caught_in_its_case(mutant):
    cid, what = MUTANTS[mutant]
    c = BY_ID[cid]
    ratios, fails = run_case(c, False, mutant)
    print(mutant, cid, {k: f"{v:.3g}" for k, v in ratios.items()}, fails[:2])
    assert fails and any(f.startswith(what) for f in fails), (ratios, fails)
    assert run_case(c, False)[1] == []


def test_a_repeated_forward_trip_is_caught():
    c = BY_ID["fp32-131081x8-add-map-acc1-nocopy"]
    ratios, fails = run_case(c, False, "trip_repeats")
    assert any(f.startswith("y") for f in fails) and math.isinf(ratios["y"])


def test_mutants_fail_the_exactness_checks_too():
    c = BY_ID["fp32-130x388-ln-all-acc1-nocopy"]
    assert any(f.startswith("dgamma") for f in run_case(c, False, "second_stage_drops_tail", exact=True)[1])
    c = BY_ID["fp32-5x256-add-map-acc1-copy"]
    assert any(f.startswith("dx") for f in run_case(c, False, "s1_of_dy", exact=True)[1])
    c = BY_ID["fp32-17x132-add-map-acc1-copy"]
    assert any(f.startswith("dbeta") for f in run_case(c, False, "dead_group_adds", exact=True)[1])
