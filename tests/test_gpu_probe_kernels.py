"""mae_batchnorm_fwd and mae_lars_step on the MI355X against the fp64 reference of tests/probe_ref.py, per element, inside the bounds
its docstring derives; the exact cases (a constant column, integer data), in place, bit-equal repeats, untracked statistics and every
refusal."""
import math

import numpy as np
import pytest
import torch

from tests import probe_ref as R

pytestmark = pytest.mark.gpu

EPS, MOM = 1e-6, 0.1
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------
# BatchNorm
# ------------------------------------------------------------------------------------------------------------------
def run_bn(dev, x, training, rm=None, rv=None, eps=EPS, mom=MOM, inplace=False, rows=None, dim=None, scratch_bytes=None, expect_ok=True):
    """One call; -> dict(rc, msg, y, mean, rstd, rm, rv) with the outputs as numpy arrays (NaN-prefilled where the call may not write)."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    rows = x.shape[0] if rows is None else rows
    dim = x.shape[1] if dim is None else dim
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    yd = xd if inplace else torch.full_like(xd, NAN)
    width = max(dim, x.shape[1])
    mean, rstd = torch.full((width,), NAN, device=dev), torch.full((width,), NAN, device=dev)
    rmd = torch.from_numpy(np.array(rm, dtype=np.float32)).to(dev) if rm is not None else None
    rvd = torch.from_numpy(np.array(rv, dtype=np.float32)).to(dev) if rv is not None else None
    need = lib.mae_batchnorm_scratch_bytes(rows, dim)
    n = max(need, 16) if scratch_bytes is None else scratch_bytes
    scratch = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    rc = lib.mae_batchnorm_fwd(_ptr(xd), rows, dim, eps, int(training), mom, _ptr(rmd), _ptr(rvd), _ptr(yd), _ptr(mean), _ptr(rstd), _ptr(scratch), n,
                               _stream(dev))
    msg = lib.mae_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    if expect_ok:
        assert rc == 0, msg
    return dict(rc=rc, msg=msg, y=yd.cpu().numpy(), mean=mean.cpu().numpy(), rstd=rstd.cpu().numpy(), rm=None if rmd is None else rmd.cpu().numpy(),
                rv=None if rvd is None else rvd.cpu().numpy(), x=xd.cpu().numpy())


_bn = {}


def bn_case(rows, dim):
    """Inputs and the fp64 references of one shape, computed once and shared (never modified)."""
    if (rows, dim) not in _bn:
        x = R.gen_bn(rows, dim)
        rm, rv = R.gen_running(dim)
        ref = R.bn_train(x, rm, rv, EPS, MOM)
        ev = R.bn_eval(x, rm, rv, EPS)
        _bn[(rows, dim)] = dict(x=x, rm=rm, rv=rv, ref=ref, bounds=R.bn_train_bounds(ref, rows, dim, rm, rv, EPS, MOM), ev=ev, ev_bounds=R.bn_eval_bounds(ev))
    return _bn[(rows, dim)]


@pytest.mark.parametrize("rows,dim", R.BN_SHAPES)
def test_batchnorm_training(dev, rows, dim):
    c = bn_case(rows, dim)
    out = run_bn(dev, c["x"], True, c["rm"], c["rv"])
    ref, b = c["ref"], c["bounds"]
    fails = []
    for name, got, want, bound in (("y", out["y"], ref["y"], b["y"]), ("mean_out", out["mean"], ref["mean"], b["mean"]),
                                   ("rstd_out", out["rstd"], ref["rstd"], b["rstd"]), ("running_mean", out["rm"], ref["running_mean"], b["running_mean"]),
                                   ("running_var", out["rv"], ref["running_var"], b["running_var"])):
        ratio, i = R.worst(got, want, bound)
        print(f"{rows}x{dim} {name}: worst error / bound {ratio:.3g} at flat index {i}")
        if not ratio <= 1.0:
            fails.append(f"{name}: error / bound {ratio:.3g} at flat index {i} (got {np.asarray(got).reshape(-1)[i]!r}, fp64 {np.asarray(want).reshape(-1)[i]!r})")
    k = R.const_column(dim)
    if np.any(bits(out["y"][:, k]) != 0):
        fails.append("the constant column's y is not +0 bit for bit")
    if bits(out["mean"][k]) != bits(R.CONST_VALUE):
        fails.append(f"the constant column's mean {out['mean'][k]!r} is not the constant {R.CONST_VALUE!r}")
    want = 1.0 / math.sqrt(R.f32(EPS))
    if not abs(float(out["rstd"][k]) - want) <= R.RSQRT_ULP * float(np.spacing(np.float32(want))):
        fails.append(f"the constant column's rstd {out['rstd'][k]!r} is not rsqrt(eps) within {R.RSQRT_ULP} ulp")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("rows,dim", R.BN_SHAPES)
def test_batchnorm_evaluation(dev, rows, dim):
    c = bn_case(rows, dim)
    out = run_bn(dev, c["x"], False, c["rm"], c["rv"])
    for name, got, want, bound in (("y", out["y"], c["ev"]["y"], c["ev_bounds"]["y"]), ("rstd_out", out["rstd"], c["ev"]["rstd"], c["ev_bounds"]["rstd"])):
        ratio, i = R.worst(got, want, bound)
        print(f"{rows}x{dim} eval {name}: worst error / bound {ratio:.3g}")
        assert ratio <= 1.0, (name, ratio, i)
    assert np.array_equal(bits(out["mean"]), bits(c["rm"])) and np.array_equal(bits(out["rm"]), bits(c["rm"])) and np.array_equal(bits(out["rv"]), bits(c["rv"]))
    single = run_bn(dev, c["x"][:1], False, c["rm"], c["rv"])          # one row is enough in evaluation
    assert np.array_equal(bits(single["y"]), bits(out["y"][:1]))


@pytest.mark.parametrize("rows,dim", [(2, 4), (256, 148), (1024, 1024)])
def test_batchnorm_integer_data_gives_the_exact_mean(dev, rows, dim):
    x = R.gen_bn_exact(rows, dim)
    ref = R.bn_train(x)
    out = run_bn(dev, x, True)
    assert np.array_equal(out["mean"].astype(np.float64), ref["mean"])


@pytest.mark.parametrize("rows,dim", R.BN_SHAPES)
def test_batchnorm_in_place_repeat_and_untracked(dev, rows, dim):
    c = bn_case(rows, dim)
    a = run_bn(dev, c["x"], True, c["rm"], c["rv"])
    for other in (run_bn(dev, c["x"], True, c["rm"], c["rv"]), run_bn(dev, c["x"], True, c["rm"], c["rv"], inplace=True)):
        for k in ("y", "mean", "rstd", "rm", "rv"):
            assert np.array_equal(bits(a[k]), bits(other[k])), k       # two runs, and in place: the same bits
    assert np.array_equal(bits(a["x"]), bits(c["x"]))                  # out of place leaves x alone
    free = run_bn(dev, c["x"], True, None, None)
    for k in ("y", "mean", "rstd"):
        assert np.array_equal(bits(a[k]), bits(free[k])), k            # NULL running buffers: the outputs as before
    e = run_bn(dev, c["x"], False, c["rm"], c["rv"])
    e2 = run_bn(dev, c["x"], False, c["rm"], c["rv"], inplace=True)
    assert np.array_equal(bits(e["y"]), bits(e2["y"]))


def test_batchnorm_refusals(dev):
    rm, rv = R.gen_running(1028)
    x = R.gen_bn(4, 1028)
    need = R.bn_geometry(4, 8)["scratch_bytes"]
    cases = [("rows = 1 in training", dict(x=x[:1, :8], training=True, rm=rm[:8], rv=rv[:8]), "rows"),
             ("dim = 6", dict(x=x[:, :8], training=True, rm=rm[:8], rv=rv[:8], dim=6), "dim"),
             ("dim = 1028", dict(x=x, training=True, rm=rm, rv=rv), "dim"),
             ("no running buffers in evaluation", dict(x=x[:, :8], training=False), "running_mean"),
             ("one running buffer", dict(x=x[:, :8], training=True, rm=rm[:8]), "running_mean"),
             ("short scratch", dict(x=x[:, :8], training=True, rm=rm[:8], rv=rv[:8], scratch_bytes=need - 16), "scratch_bytes")]
    for what, kw, word in cases:
        out = run_bn(dev, expect_ok=False, **kw)
        assert out["rc"] != 0 and word in out["msg"], (what, out["rc"], out["msg"])
        assert np.all(np.isnan(out["y"])) and np.all(np.isnan(out["mean"])) and np.all(np.isnan(out["rstd"])), what
        if out["rm"] is not None:
            assert np.array_equal(bits(out["rm"]), bits(kw["rm"])), what
        if out["rv"] is not None:
            assert np.array_equal(bits(out["rv"]), bits(kw["rv"])), what
    ok = run_bn(dev, x[:, :8], True, rm[:8], rv[:8], scratch_bytes=need)   # exactly what the size function asks for is enough
    assert ok["rc"] == 0 and np.all(np.isfinite(ok["y"]))


# ------------------------------------------------------------------------------------------------------------------
# LARS
# ------------------------------------------------------------------------------------------------------------------
LR, MOMENTUM, TRUST = 0.78, 0.9, 0.001
COUNTS = [4, 1440, 131072, R.LARS_WRAP + 1024]   # the minimum, 10 x 144, 128 x 1024, one count past a single grid pass of the norm kernel


def run_lars(dev, p, g, mu, adapt, wd, count=None, norms=True):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    pd, gd, md = (torch.from_numpy(np.ascontiguousarray(t)).to(dev) for t in (p, g, mu))
    nd = torch.full((2,), NAN, device=dev) if norms else None
    scratch = torch.empty(4096, dtype=torch.float32, device=dev)
    check(lib.mae_lars_step(_ptr(pd), _ptr(gd), _ptr(md), p.size if count is None else count, adapt, LR, MOMENTUM, wd, TRUST, _ptr(nd), _ptr(scratch),
                            _stream(dev)))
    torch.cuda.synchronize()
    return pd.cpu().numpy(), md.cpu().numpy(), gd.cpu().numpy(), None if nd is None else nd.cpu().numpy()


_lars = {}


def lars_inputs(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _lars:
        _lars[key] = R.gen_lars(n, 3, **kw)
    return _lars[key]


def check_lars(dev, n, adapt, wd, **kw):
    p, g, mu = lars_inputs(n, **kw)
    ref = R.lars_step(p, g, mu, adapt, LR, MOMENTUM, wd, TRUST)
    b = R.lars_bounds(ref, n)
    p2, mu2, g2, norms = run_lars(dev, p, g, mu, adapt, wd)
    rp, _ = R.worst(p2, ref["p"], b["p"])
    rmu, _ = R.worst(mu2, ref["mu"], b["mu"])
    rn = max(abs(float(norms[0]) - ref["pn"]) / b["pn"] if b["pn"] > 0 else float(norms[0] != 0), abs(float(norms[1]) - ref["un"]) / b["un"]
             if b["un"] > 0 else float(norms[1] != 0))
    print(f"n {n} adapt {adapt} wd {wd} {kw}: p {rp:.3g} mu {rmu:.3g} norms {rn:.3g} (error / bound), q {ref['q']:.6g}")
    assert rp <= 1.0 and rmu <= 1.0 and rn <= 1.0
    assert np.array_equal(bits(g2), bits(g))
    again = run_lars(dev, p, g, mu, adapt, wd)
    assert np.array_equal(bits(p2), bits(again[0])) and np.array_equal(bits(mu2), bits(again[1])) and np.array_equal(bits(norms), bits(again[3]))
    quiet = run_lars(dev, p, g, mu, adapt, wd, norms=False)                  # norms_out = NULL changes nothing else
    assert np.array_equal(bits(p2), bits(quiet[0])) and np.array_equal(bits(mu2), bits(quiet[1]))
    return ref


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("adapt", [1, 0])
@pytest.mark.parametrize("zero_mu", [True, False])
@pytest.mark.parametrize("wd", [0.0, 0.05])
def test_lars_step(dev, n, adapt, zero_mu, wd):
    ref = check_lars(dev, n, adapt, wd, zero_mu=zero_mu)
    assert (ref["q"] != 1.0) == bool(adapt)


@pytest.mark.parametrize("n", [4, 1440])
def test_lars_zero_norms_give_no_trust_ratio(dev, n):
    assert check_lars(dev, n, 1, 0.05, zero_p=True)["q"] == 1.0
    assert check_lars(dev, n, 1, 0.0, zero_g=True)["q"] == 1.0


def test_lars_count_zero_touches_nothing(dev):
    p, g, mu = lars_inputs(1440)
    p2, mu2, g2, norms = run_lars(dev, p, g, mu, 1, 0.05, count=0)
    assert np.array_equal(bits(p2), bits(p)) and np.array_equal(bits(mu2), bits(mu)) and np.array_equal(bits(g2), bits(g)) and np.all(np.isnan(norms))


def test_lars_refuses_a_count_that_is_no_multiple_of_four(dev):
    from ssrl_vit_mae_jepa_amd._lib import MaeHipError
    p, g, mu = lars_inputs(1440)
    with pytest.raises(MaeHipError, match="count"):
        run_lars(dev, p, g, mu, 1, 0.0, count=6)
