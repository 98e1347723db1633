"""The attentive probe's kernels (k_attnpool.hip) and mae_batchnorm_stats on the MI355X against the fp64 reference of
tests/attnpool_ref.py, per element, inside the bounds its docstring derives; the edge cases of the softmax, bit-equal repeats, an image
alone and inside a batch, untouched inputs and every refusal."""
import math

import numpy as np
import pytest
import torch

from tests import attnpool_ref as R
from tests import probe_ref as P

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


def up(dev, a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def call(fn, *args):
    """rc and message of one library call, synchronised."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    rc = fn(*args)
    msg = lib.mae_last_error().decode() if rc else ""
    torch.cuda.synchronize()
    return rc, msg


def run_fwd(dev, x, mean, uq, H, B=None, T=None, D=None, shift=None):
    """mae_attn_pool_fwd -> dict(rc, msg, ybar, lse, x); outputs NaN-prefilled.  B / T / D / H override what the call is told;
    shift names one buffer that is passed 4 bytes off a 16-byte boundary."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    b, t, d = x.shape
    xd, md, ud = up(dev, x), up(dev, mean), up(dev, uq)
    ybar, lse = torch.full((b * uq.shape[0] * d + 4,), NAN, device=dev), torch.full((b * uq.shape[0] + 4,), NAN, device=dev)
    if shift == "x":
        xd = torch.cat([xd.reshape(-1), xd.new_zeros(4)])[1:]
    yv = ybar[1:] if shift == "ybar" else ybar
    rc, msg = call(lib.mae_attn_pool_fwd, _ptr(xd), _ptr(md), _ptr(ud), b if B is None else B, t if T is None else T, d if D is None else D, H,
                   _ptr(yv), _ptr(lse), _stream(dev))
    return dict(rc=rc, msg=msg, ybar=ybar[:b * uq.shape[0] * d].cpu().numpy().reshape(b, uq.shape[0], d), lse=lse[:b * uq.shape[0]].cpu().numpy().reshape(b, -1),
                x=xd.cpu().numpy().reshape(-1)[:x.size].reshape(x.shape) if shift != "x" else x)


def run_bwd(dev, x, mean, uq, lse, ybar, g, H, B=None, T=None, D=None, scratch_bytes=None):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    b, t, d = x.shape
    xd, md, ud, ld, yd, gd = (up(dev, a) for a in (x, mean, uq, lse, ybar, g))
    duq = torch.full(uq.shape, NAN, device=dev)
    need = lib.mae_attn_pool_bwd_scratch_bytes(b, t, d, uq.shape[0])
    assert need == R.geometry(d, uq.shape[0], t, b)["bwd_scratch_bytes"]
    n = need if scratch_bytes is None else scratch_bytes
    scratch = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    rc, msg = call(lib.mae_attn_pool_bwd, _ptr(xd), _ptr(md), _ptr(ud), _ptr(ld), _ptr(yd), _ptr(gd), b if B is None else B, t if T is None else T,
                   d if D is None else D, H, _ptr(duq), _ptr(scratch), n, _stream(dev))
    return dict(rc=rc, msg=msg, duq=duq.cpu().numpy(), x=xd.cpu().numpy())


def run_fold(dev, q, wk, rstd, H, D=None):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    uq = torch.full((max(H, 1), q.size), NAN, device=dev)
    rc, msg = call(lib.mae_attn_probe_fold, _ptr(up(dev, q)), _ptr(up(dev, wk)), _ptr(up(dev, rstd)), q.size if D is None else D, H, _ptr(uq), _stream(dev))
    return dict(rc=rc, msg=msg, uq=uq.cpu().numpy())


def run_fold_bwd(dev, duq, q, wk, rstd, H, D=None):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    dq, dwk = torch.full(q.shape, NAN, device=dev), torch.full(wk.shape, NAN, device=dev)
    rc, msg = call(lib.mae_attn_probe_fold_bwd, _ptr(up(dev, duq)), _ptr(up(dev, q)), _ptr(up(dev, wk)), _ptr(up(dev, rstd)), q.size if D is None else D, H,
                   _ptr(dq), _ptr(dwk), _stream(dev))
    return dict(rc=rc, msg=msg, dq=dq.cpu().numpy(), dwk=dwk.cpu().numpy())


def run_project(dev, ybar, rstd, wv, H, D=None):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    b, _, d = ybar.shape
    p = torch.full((b, d), NAN, device=dev)
    rc, msg = call(lib.mae_attn_probe_project, _ptr(up(dev, ybar)), _ptr(up(dev, rstd)), _ptr(up(dev, wv)), b, d if D is None else D, H, _ptr(p), _stream(dev))
    return dict(rc=rc, msg=msg, p=p.cpu().numpy())


def run_project_bwd(dev, dp, ybar, rstd, wv, H, D=None, scratch_bytes=None):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    b, h, d = ybar.shape
    g, dwv = torch.full(ybar.shape, NAN, device=dev), torch.full(wv.shape, NAN, device=dev)
    need = lib.mae_attn_probe_project_bwd_scratch_bytes(b, d, h)
    assert need == R.geometry(d, h, 1, b)["wv_slices"] * d * d * 4
    n = need if scratch_bytes is None else scratch_bytes
    scratch = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    rc, msg = call(lib.mae_attn_probe_project_bwd, _ptr(up(dev, dp)), _ptr(up(dev, ybar)), _ptr(up(dev, rstd)), _ptr(up(dev, wv)), b,
                   d if D is None else D, H, _ptr(g), _ptr(dwv), _ptr(scratch), n, _stream(dev))
    return dict(rc=rc, msg=msg, g=g.cpu().numpy(), dwv=dwv.cpu().numpy())


_cases = {}


def case(B, T, D, H):
    """Inputs of one shape, generated once and shared (never modified)."""
    if (B, T, D, H) not in _cases:
        _cases[(B, T, D, H)] = R.gen_case(B, T, D, H)
    return _cases[(B, T, D, H)]


def judge(tag, fails, name, got, want, bound):
    ratio, i = R.worst(got, want, bound)
    print(f"{tag} {name}: worst error / bound {ratio:.3g} at flat index {i}")
    if not ratio <= 1.0:
        fails.append(f"{name}: error / bound {ratio:.3g} at flat index {i} (got {np.asarray(got).reshape(-1)[i]!r}, fp64 {np.asarray(want).reshape(-1)[i]!r})")


@pytest.mark.parametrize("B,T,D,H", R.kernel_cases())
def test_every_kernel_inside_its_bound(dev, B, T, D, H):
    c = case(B, T, D, H)
    tag, fails = f"{B}x{T}x{D} H{H}", []
    fo = run_fold(dev, c["q"], c["wk"], c["rstd"], H)
    assert fo["rc"] == 0, fo["msg"]
    uq = fo["uq"]
    judge(tag, fails, "uq", uq, R.fold(c["q"], c["wk"], c["rstd"], H), R.fold_bound(c["q"], c["wk"], c["rstd"], H))
    fw = run_fwd(dev, c["x"], c["mean"], uq, H)
    assert fw["rc"] == 0, fw["msg"]
    ref = R.pool_fwd(c["x"], c["mean"], uq)
    b = R.pool_fwd_bounds(ref, uq, True, H)
    judge(tag, fails, "ybar", fw["ybar"], ref["ybar"], b["ybar"])
    judge(tag, fails, "lse", fw["lse"], ref["lse"], b["lse"])
    ybar, lse = fw["ybar"], fw["lse"]
    pr = run_project(dev, ybar, c["rstd"], c["wv"], H)
    assert pr["rc"] == 0, pr["msg"]
    judge(tag, fails, "p", pr["p"], R.project(ybar, c["rstd"], c["wv"], H), R.project_bound(ybar, c["rstd"], c["wv"], H))
    pb = run_project_bwd(dev, c["dp"], ybar, c["rstd"], c["wv"], H)
    assert pb["rc"] == 0, pb["msg"]
    rpb, bpb = R.project_bwd(c["dp"], ybar, c["rstd"], c["wv"], H), R.project_bwd_bounds(c["dp"], ybar, c["rstd"], c["wv"], H)
    judge(tag, fails, "g", pb["g"], rpb["g"], bpb["g"])
    judge(tag, fails, "dwv", pb["dwv"], rpb["dwv"], bpb["dwv"])
    g = pb["g"]
    bw = run_bwd(dev, c["x"], c["mean"], uq, lse, ybar, g, H)
    assert bw["rc"] == 0, bw["msg"]
    rbw = R.pool_bwd(c["x"], c["mean"], uq, lse, ybar, g)
    judge(tag, fails, "duq", bw["duq"], rbw["duq"], R.pool_bwd_bounds(rbw, uq, lse, ybar, g, True, H))
    fb = run_fold_bwd(dev, bw["duq"], c["q"], c["wk"], c["rstd"], H)
    assert fb["rc"] == 0, fb["msg"]
    rfb, bfb = R.fold_bwd(bw["duq"], c["q"], c["wk"], c["rstd"], H), R.fold_bwd_bounds(bw["duq"], c["q"], c["wk"], c["rstd"], H)
    judge(tag, fails, "dq", fb["dq"], rfb["dq"], bfb["dq"])
    judge(tag, fails, "dwk", fb["dwk"], rfb["dwk"], bfb["dwk"])
    # two runs give equal bits; the token buffer is as it was
    fw2, bw2 = run_fwd(dev, c["x"], c["mean"], uq, H), run_bwd(dev, c["x"], c["mean"], uq, lse, ybar, g, H)
    if not (np.array_equal(bits(fw["ybar"]), bits(fw2["ybar"])) and np.array_equal(bits(fw["lse"]), bits(fw2["lse"]))):
        fails.append("two forward runs differ in bits")
    if not np.array_equal(bits(bw["duq"]), bits(bw2["duq"])):
        fails.append("two backward runs differ in bits")
    if not (np.array_equal(bits(fw["x"]), bits(c["x"])) and np.array_equal(bits(bw["x"]), bits(c["x"]))):
        fails.append("the token buffer changed")
    # an image alone and inside the batch: the same bits
    if B > 1:
        j = B // 2
        one = run_fwd(dev, c["x"][j:j + 1], c["mean"], uq, H)
        if not (np.array_equal(bits(one["ybar"][0]), bits(fw["ybar"][j])) and np.array_equal(bits(one["lse"][0]), bits(fw["lse"][j]))):
            fails.append(f"image {j} alone and inside the batch differ in bits")
    assert not fails, "\n".join(fails)


EDGE = [(3, 145, 384, 6), (2, 65, 64, 1), (2, 257, 1024, 16)]


@pytest.mark.parametrize("B,T,D,H", EDGE)
def test_zero_query_gives_the_centred_mean(dev, B, T, D, H):
    c = case(B, T, D, H)
    uq = np.zeros((H, D), dtype=np.float32)
    out = run_fwd(dev, c["x"], c["mean"], uq, H)
    assert out["rc"] == 0, out["msg"]
    ref = R.pool_fwd(c["x"], c["mean"], uq)
    assert np.allclose(ref["a"], 1.0 / T, rtol=1e-12)
    b = R.pool_fwd_bounds(ref, uq, True, H)
    centred = (c["x"].astype(np.float64) - c["mean"].astype(np.float64)).mean(1)
    ry, _ = R.worst(out["ybar"], np.broadcast_to(centred[:, None, :], ref["ybar"].shape), b["ybar"])
    rl, _ = R.worst(out["lse"], np.full_like(ref["lse"], math.log(T)), b["lse"])
    print(f"{B}x{T}x{D} H{H} zero query: ybar {ry:.3g} lse {rl:.3g} (error / bound)")
    assert ry <= 1.0 and rl <= 1.0


@pytest.mark.parametrize("B,T,D,H", EDGE)
def test_one_token_200_above_the_rest(dev, B, T, D, H):
    c = case(B, T, D, H)
    uq = (R.fold(c["q"], c["wk"], c["rstd"], H) * 0.05).astype(np.float32)
    x = c["x"].copy()
    step = np.linalg.pinv(uq.astype(np.float64)) @ np.full(H, 1.0)                    # uq @ step = 1 for every head
    s = R.pool_fwd(x, c["mean"], uq)["s"]
    tstar = [(7 * b + 3) % T for b in range(B)]
    for b in range(B):
        lift = 200.0 + s[b].max() - s[b, tstar[b]].min()
        x[b, tstar[b]] = (x[b, tstar[b]] + lift * step).astype(np.float32)
    ref = R.pool_fwd(x, c["mean"], uq)
    for b in range(B):
        rest = np.delete(ref["s"][b], tstar[b], axis=0)
        assert np.all(ref["s"][b, tstar[b]] - rest.max(0) >= 199.0)
    out = run_fwd(dev, x, c["mean"], uq, H)
    assert out["rc"] == 0, out["msg"]
    assert np.all(np.isfinite(out["ybar"])) and np.all(np.isfinite(out["lse"]))
    bnd = R.pool_fwd_bounds(ref, uq, True, H)
    token = np.stack([ref["c"][b, tstar[b]] for b in range(B)])[:, None, :]
    ry, _ = R.worst(out["ybar"], np.broadcast_to(token, ref["ybar"].shape), bnd["ybar"])
    rl, _ = R.worst(out["lse"], ref["lse"], bnd["lse"])
    print(f"{B}x{T}x{D} H{H} spike: ybar {ry:.3g} lse {rl:.3g} (error / bound)")
    assert ry <= 1.0 and rl <= 1.0
    g = (np.random.default_rng(3).standard_normal((B, H, D)) * 1e-2).astype(np.float32)
    bw = run_bwd(dev, x, c["mean"], uq, out["lse"], out["ybar"], g, H)
    assert bw["rc"] == 0 and np.all(np.isfinite(bw["duq"])), bw["msg"]
    rbw = R.pool_bwd(x, c["mean"], uq, out["lse"], out["ybar"], g)
    rd, _ = R.worst(bw["duq"], rbw["duq"], R.pool_bwd_bounds(rbw, uq, out["lse"], out["ybar"], g, True, H))
    print(f"{B}x{T}x{D} H{H} spike: duq {rd:.3g}")
    assert rd <= 1.0


@pytest.mark.parametrize("B,T,D,H", EDGE)
def test_scores_of_magnitude_1e4_and_no_mean(dev, B, T, D, H):
    c = case(B, T, D, H)
    uq0 = R.fold(c["q"], c["wk"], c["rstd"], H)
    for mean in (c["mean"], None):
        smax = np.abs(R.pool_fwd(c["x"], mean, uq0)["s"]).max()
        for scale, what in ((1e4 / smax, "1e4"), (1.0, "plain")):
            if mean is not None and what == "plain":
                continue   # test_every_kernel_inside_its_bound has it
            uq = (uq0 * scale).astype(np.float32)
            ref = R.pool_fwd(c["x"], mean, uq)
            out = run_fwd(dev, c["x"], mean, uq, H)
            assert out["rc"] == 0 and np.all(np.isfinite(out["ybar"])) and np.all(np.isfinite(out["lse"])), out["msg"]
            b = R.pool_fwd_bounds(ref, uq, mean is not None, H)
            ry, _ = R.worst(out["ybar"], ref["ybar"], b["ybar"])
            rl, _ = R.worst(out["lse"], ref["lse"], b["lse"])
            g = (np.random.default_rng(4).standard_normal((B, H, D)) * 1e-2).astype(np.float32)
            bw = run_bwd(dev, c["x"], mean, uq, out["lse"], out["ybar"], g, H)
            assert bw["rc"] == 0, bw["msg"]
            rbw = R.pool_bwd(c["x"], mean, uq, out["lse"], out["ybar"], g)
            rd, _ = R.worst(bw["duq"], rbw["duq"], R.pool_bwd_bounds(rbw, uq, out["lse"], out["ybar"], g, mean is not None, H))
            print(f"{B}x{T}x{D} H{H} scores {what}, mean {'given' if mean is not None else 'NULL'}: ybar {ry:.3g} lse {rl:.3g} duq {rd:.3g} (error / bound)")
            assert ry <= 1.0 and rl <= 1.0 and rd <= 1.0


# ------------------------------------------------------------------------------------------------------------------
# mae_batchnorm_stats
# ------------------------------------------------------------------------------------------------------------------
def run_bn(dev, fn_name, x, training, rm, rv, rows=None, dim=None, scratch_bytes=None, eps=1e-6, mom=0.1):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    rows = x.shape[0] if rows is None else rows
    dim = x.shape[1] if dim is None else dim
    xd = up(dev, x)
    width = max(dim, x.shape[1])
    mean, rstd = torch.full((width,), NAN, device=dev), torch.full((width,), NAN, device=dev)
    rmd, rvd = up(dev, rm), up(dev, rv)
    need = lib.mae_batchnorm_scratch_bytes(rows, dim)
    n = max(need, 16) if scratch_bytes is None else scratch_bytes
    scratch = torch.empty(max(n, 16), dtype=torch.uint8, device=dev)
    if fn_name == "fwd":
        y = torch.full_like(xd, NAN)
        rc, msg = call(lib.mae_batchnorm_fwd, _ptr(xd), rows, dim, eps, int(training), mom, _ptr(rmd), _ptr(rvd), _ptr(y), _ptr(mean), _ptr(rstd),
                       _ptr(scratch), n, _stream(dev))
    else:
        rc, msg = call(lib.mae_batchnorm_stats, _ptr(xd), rows, dim, eps, int(training), mom, _ptr(rmd), _ptr(rvd), _ptr(mean), _ptr(rstd), _ptr(scratch), n,
                       _stream(dev))
    return dict(rc=rc, msg=msg, mean=mean.cpu().numpy(), rstd=rstd.cpu().numpy(), rm=None if rmd is None else rmd.cpu().numpy(),
                rv=None if rvd is None else rvd.cpu().numpy(), x=xd.cpu().numpy())


@pytest.mark.parametrize("rows,dim", P.BN_SHAPES)
def test_batchnorm_stats_has_the_bits_of_batchnorm_fwd(dev, rows, dim):
    x = P.gen_bn(rows, dim)
    rm, rv = P.gen_running(dim)
    for training in (True, False):
        a, b = run_bn(dev, "fwd", x, training, rm, rv), run_bn(dev, "stats", x, training, rm, rv)
        assert a["rc"] == 0 and b["rc"] == 0, (a["msg"], b["msg"])
        for k in ("mean", "rstd", "rm", "rv"):
            assert np.array_equal(bits(a[k]), bits(b[k])), (training, k)
        assert np.array_equal(bits(b["x"]), bits(x))
    out = run_bn(dev, "stats", x, True, rm, rv)
    ref = P.bn_train(x, rm, rv, 1e-6, 0.1)
    bnd = P.bn_train_bounds(ref, rows, dim, rm, rv, 1e-6, 0.1)
    for name, got, want, bound in (("mean_out", out["mean"], ref["mean"], bnd["mean"]), ("rstd_out", out["rstd"], ref["rstd"], bnd["rstd"]),
                                   ("running_mean", out["rm"], ref["running_mean"], bnd["running_mean"]),
                                   ("running_var", out["rv"], ref["running_var"], bnd["running_var"])):
        ratio, i = P.worst(got, want, bound)
        print(f"{rows}x{dim} stats {name}: worst error / bound {ratio:.3g}")
        assert ratio <= 1.0, (name, ratio, i)


def test_batchnorm_stats_refusals(dev):
    rm, rv = P.gen_running(1028)
    x = P.gen_bn(4, 1028)
    need = P.bn_geometry(4, 8)["scratch_bytes"]
    cases = [("rows = 1 in training", dict(x=x[:1, :8], training=True, rm=rm[:8], rv=rv[:8]), "rows"),
             ("dim = 6", dict(x=x[:, :8], training=True, rm=rm[:8], rv=rv[:8], dim=6), "dim"),
             ("dim = 1028", dict(x=x, training=True, rm=rm, rv=rv), "dim"),
             ("no running buffers in evaluation", dict(x=x[:, :8], training=False, rm=None, rv=None), "running_mean"),
             ("short scratch", dict(x=x[:, :8], training=True, rm=rm[:8], rv=rv[:8], scratch_bytes=need - 16), "scratch_bytes")]
    for what, kw, word in cases:
        out = run_bn(dev, "stats", **kw)
        assert out["rc"] != 0 and word in out["msg"], (what, out["rc"], out["msg"])
        assert np.all(np.isnan(out["mean"])) and np.all(np.isnan(out["rstd"])), what
        if out["rm"] is not None:
            assert np.array_equal(bits(out["rm"]), bits(kw["rm"])) and np.array_equal(bits(out["rv"]), bits(kw["rv"])), what


# ------------------------------------------------------------------------------------------------------------------
# refusals: nothing is launched, nothing is written
# ------------------------------------------------------------------------------------------------------------------
def test_pool_refusals(dev):
    B, T, D, H = 2, 5, 64, 4
    c = case(B, T, D, H)
    uq = R.fold(c["q"], c["wk"], c["rstd"], H).astype(np.float32)
    ok = run_fwd(dev, c["x"], c["mean"], uq, H)
    assert ok["rc"] == 0
    g = np.ones((B, H, D), dtype=np.float32)
    limits = [("dim = 6", dict(D=6), "dim"), ("dim = 1028", dict(D=1028), "dim"), ("dim = 0", dict(D=0), "dim"), ("heads = 0", dict(H=0), "heads"),
              ("heads = 17", dict(H=17), "heads"), ("heads = 3 does not divide 64", dict(H=3), "heads"), ("tokens = 0", dict(T=0), "tokens"),
              ("batch = 0", dict(B=0), "batch"), ("batch * tokens = 2^31", dict(B=2 ** 16, T=2 ** 15), "2^31")]
    for what, kw, word in limits:
        kw = dict(kw)
        heads = kw.pop("H", H)
        out = run_fwd(dev, c["x"], c["mean"], uq, heads, **kw)
        assert out["rc"] != 0 and word in out["msg"], (what, out["rc"], out["msg"])
        assert np.all(np.isnan(out["ybar"])) and np.all(np.isnan(out["lse"])), what
        out = run_bwd(dev, c["x"], c["mean"], uq, ok["lse"], ok["ybar"], g, heads, **kw)
        assert out["rc"] != 0 and word in out["msg"], (what, out["rc"], out["msg"])
        assert np.all(np.isnan(out["duq"])), what
        from ssrl_vit_mae_jepa_amd._lib import lib
        assert lib.mae_attn_pool_bwd_scratch_bytes(kw.get("B", B), kw.get("T", T), kw.get("D", D), heads) == -1, what
    for shift in ("x", "ybar"):
        out = run_fwd(dev, c["x"], c["mean"], uq, H, shift=shift)
        assert out["rc"] != 0 and "aligned" in out["msg"], (shift, out["msg"])
        assert np.all(np.isnan(out["ybar"])) and np.all(np.isnan(out["lse"])), shift
    need = R.geometry(D, H, T, B)["bwd_scratch_bytes"]
    out = run_bwd(dev, c["x"], c["mean"], uq, ok["lse"], ok["ybar"], g, H, scratch_bytes=need - 16)
    assert out["rc"] != 0 and "scratch_bytes" in out["msg"] and np.all(np.isnan(out["duq"]))
    out = run_bwd(dev, c["x"], c["mean"], uq, ok["lse"], ok["ybar"], g, H, scratch_bytes=need)   # exactly the query's size is enough
    assert out["rc"] == 0 and np.all(np.isfinite(out["duq"]))


def test_small_piece_refusals(dev):
    B, T, D, H = 2, 5, 64, 4
    c = case(B, T, D, H)
    ybar = np.ones((B, H, D), dtype=np.float32)
    duq = np.ones((H, D), dtype=np.float32)
    from ssrl_vit_mae_jepa_amd._lib import lib
    for what, kw, word in [("dim = 6", dict(D=6), "dim"), ("dim = 1028", dict(D=1028), "dim"), ("heads = 0", dict(H=0), "heads"),
                           ("heads = 17", dict(H=17), "heads"), ("heads = 3", dict(H=3), "heads")]:
        kw = dict(kw)
        heads = kw.pop("H", H)
        out = run_fold(dev, c["q"], c["wk"], c["rstd"], heads, **kw)
        assert out["rc"] != 0 and word in out["msg"] and np.all(np.isnan(out["uq"])), (what, out["msg"])
        out = run_fold_bwd(dev, duq, c["q"], c["wk"], c["rstd"], heads, **kw)
        assert out["rc"] != 0 and word in out["msg"] and np.all(np.isnan(out["dq"])) and np.all(np.isnan(out["dwk"])), (what, out["msg"])
        out = run_project(dev, ybar, c["rstd"], c["wv"], heads, **kw)
        assert out["rc"] != 0 and word in out["msg"] and np.all(np.isnan(out["p"])), (what, out["msg"])
        out = run_project_bwd(dev, c["dp"], ybar, c["rstd"], c["wv"], heads, **kw)
        assert out["rc"] != 0 and word in out["msg"] and np.all(np.isnan(out["g"])) and np.all(np.isnan(out["dwv"])), (what, out["msg"])
        assert lib.mae_attn_probe_project_bwd_scratch_bytes(B, kw.get("D", D), heads) == -1, what
    need = lib.mae_attn_probe_project_bwd_scratch_bytes(B, D, H)
    out = run_project_bwd(dev, c["dp"], ybar, c["rstd"], c["wv"], H, scratch_bytes=need - 16)
    assert out["rc"] != 0 and "scratch_bytes" in out["msg"] and np.all(np.isnan(out["g"])) and np.all(np.isnan(out["dwv"]))
