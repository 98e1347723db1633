"""features_kernel (k_representation.hip) through mae_features_tap against mae_features_pool and tests/engine_kernels_ref.py (-m gpu).

Both entries launch the one kernel: mae_features_tap picks the rows by (with_cls, pool), adds a row stride on the output and a fourth
pool, so its reference is mae_features_pool's own output: every case of engine_kernels_ref.pool_cases() is written into slot 1 of a NaN-filled (B, 3, D + 4) buffer and must hold
mae_features_pool's bits, stay inside expect_pool's bound, and leave slots 0 and 2 and the 4 padding columns NaN.  A case whose rows
[lo, hi) are not a pool of the whole sequence (the class row, the patch rows, every row) runs image by image on the view of those
rows as a patch-only sequence: mae_features_pool's result for an image does not depend on its batch (test_gpu_engine_kernels.py).
MAE_POOL_CLS_MEAN_PATCHES = [class row | patch mean] must equal the two single pools bit for bit.  Extra shapes: one patch row behind
the class row (three idle waves), 4 and 5 patch rows (a ragged partition), D = 32 and 320 (a partial last lane vector), D = 1024.
The last test prints the worst error / bound.  About 2 s on an MI355X."""
import numpy as np
import pytest
import torch

from tests import engine_kernels_ref as R
from tests.test_gpu_token_kernels import up
from tests.util import _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1}                    # MAE_F32, MAE_BF16
CLS, MEAN, MEAN_PATCHES, CLS_MEAN = 0, 1, 2, 3  # MAE_POOL_*
PAD = 4                                       # columns between two slices that nobody may write
POOL = {c.id: c for c in R.pool_cases()}
POOL_GROUPS = sorted({(c.D, c.seq, c.lo, c.hi) for c in POOL.values()})
EXTRA_SHAPES = ((2, 32), (5, 320), (6, 32), (6, 320), (5, 8), (2, 1024), (10, 1024))   # (seq, D)
WORST = {}


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def bits(t):
    return t.contiguous().view(torch.int32)


def pool_out(c, t, lo, hi, s, dev):
    """mae_features_pool over rows [lo, hi): (B, D) on the device."""
    out = up(R.nan_buf(c.B, c.D), dev)
    check(lib.mae_features_pool(_ptr(t["x"]), _ptr(t["branch"]), DT[c.dtype], _ptr(t["gamma"]), _ptr(t["beta"]), R.EPS, c.B, c.seq, c.D, lo, hi, int(c.l2),
                                _ptr(out), s))
    assert torch.isnan(out[c.B:]).all()
    return out[:c.B]


def tap(x, branch, c, t, B, seq, with_cls, pool, out, stride, s):
    check(lib.mae_features_tap(_ptr(x), _ptr(branch), DT[c.dtype], _ptr(t["gamma"]), _ptr(t["beta"]), R.EPS, B, seq, c.D, with_cls, pool, int(c.l2), _ptr(out),
                               stride, s))


def tap_slot(c, t, lo, hi, s, dev, pool=None):
    """Rows [lo, hi) (or `pool` of the whole sequence, class row first) by mae_features_tap into slot 1 of a NaN-filled (B, 3, W + PAD)
    buffer -> (B, W); everything else in the buffer must still be NaN."""
    W = 2 * c.D if pool == CLS_MEAN else c.D
    buf = torch.full((c.B, 3, W + PAD), float("nan"), device=dev)
    stride = 3 * (W + PAD)
    if pool is None:
        pool = {(0, c.seq): MEAN, (1, c.seq): MEAN_PATCHES, (0, 1): CLS}.get((lo, hi))
    if pool is not None:
        tap(t["x"], t["branch"], c, t, c.B, c.seq, 1, pool, buf[0, 1], stride, s)
    else:
        for b in range(c.B):   # the rows as a patch-only sequence of hi - lo rows, one image at a time
            tap(t["x"][b, lo:hi], t["branch"][b, lo:hi], c, t, 1, hi - lo, 0, MEAN, buf[b, 1], stride, s)
    torch.cuda.synchronize()
    got = buf[:, 1, :W].clone()
    buf[:, 1, :W] = float("nan")
    assert torch.isnan(buf).all(), f"{c.id}: wrote outside its slice"
    return got


def settle(c, variant, sub, d, got, fails):
    """got (B, D) on the device against expect_pool of the case `sub` (rows sub.lo .. sub.hi of the data d)."""
    init = R.pool_inits(sub)
    full = init["features_pool.out"].copy()
    full[:sub.B] = got.cpu().numpy()
    e = R.expect_pool(sub, d)
    ratios, f = R.judge(e, {"features_pool.out": full}, init)
    v = ratios["features_pool.out"]
    if variant not in WORST or v > WORST[variant][0]:
        WORST[variant] = (v, c.id)
    print(c.id, variant, f"{v:.3f}")
    fails += [f"{c.id} [{variant}] {x}" for x in f]


@pytest.mark.parametrize("group", POOL_GROUPS, ids=lambda g: "D{}-s{}r{}_{}".format(*g))
def test_tap_equals_features_pool(dev, group):
    s, fails = stream(dev), []
    for c in (c for c in POOL.values() if (c.D, c.seq, c.lo, c.hi) == group):
        d = R.gen_pool(c)
        t = {k: up(v, dev) for k, v in d.items()}
        want = pool_out(c, t, c.lo, c.hi, s, dev)
        got = tap_slot(c, t, c.lo, c.hi, s, dev)
        if not torch.equal(bits(got), bits(want)):
            fails.append(f"{c.id}: {int((bits(got) != bits(want)).sum())} elements differ from mae_features_pool")
        settle(c, f"{c.kind} {c.dtype} {'l2' if c.l2 else 'none'}", c, d, got, fails)
        if (c.lo, c.hi) == (0, c.seq):   # without a class row both means are the mean over every row
            buf = torch.full((c.B, c.D), float("nan"), device=dev)
            tap(t["x"], t["branch"], c, t, c.B, c.seq, 0, MEAN_PATCHES, buf, c.D, s)
            torch.cuda.synchronize()
            if not torch.equal(bits(buf), bits(want)):
                fails.append(f"{c.id}: MAE_POOL_MEAN_PATCHES on a patch-only sequence differs")
    assert not fails, "\n".join(fails)


def extra_cases():
    return [R.PoolCase(f"tap-s{seq}D{D}-{dt}-{'l2' if l2 else 'none'}", 3, seq, D, 0, seq, dt, l2, "random")
            for seq, D in EXTRA_SHAPES for dt in ("f32", "bf16") for l2 in (False, True)]


EXTRA = {c.id: c for c in extra_cases()}


@pytest.mark.parametrize("shape", EXTRA_SHAPES, ids=lambda g: "s{}D{}".format(*g))
def test_cls_mean_halves_and_extra_shapes(dev, shape):
    """Every pool at the shapes the partition can get wrong: the three single pools against mae_features_pool, and both halves of
    MAE_POOL_CLS_MEAN_PATCHES against MAE_POOL_CLS and MAE_POOL_MEAN_PATCHES, bit for bit; all inside expect_pool's bounds."""
    import dataclasses
    s, fails = stream(dev), []
    for c in (c for c in EXTRA.values() if (c.seq, c.D) == shape):
        d = R.gen_pool(c)
        t = {k: up(v, dev) for k, v in d.items()}
        ranges = {"cls": (0, 1), "mean": (0, c.seq), "patches": (1, c.seq)}
        want = {k: pool_out(c, t, lo, hi, s, dev) for k, (lo, hi) in ranges.items()}
        for k, (lo, hi) in ranges.items():
            got = tap_slot(c, t, lo, hi, s, dev)
            if not torch.equal(bits(got), bits(want[k])):
                fails.append(f"{c.id}: pool {k} differs from mae_features_pool")
            settle(c, f"{k} {c.dtype} {'l2' if c.l2 else 'none'}", dataclasses.replace(c, lo=lo, hi=hi), d, got, fails)
        both = tap_slot(c, t, 0, c.seq, s, dev, pool=CLS_MEAN)
        assert both.shape == (c.B, 2 * c.D)
        if not torch.equal(bits(both[:, :c.D]), bits(want["cls"])):
            fails.append(f"{c.id}: the class half of MAE_POOL_CLS_MEAN_PATCHES differs from MAE_POOL_CLS")
        if not torch.equal(bits(both[:, c.D:]), bits(want["patches"])):
            fails.append(f"{c.id}: the patch half of MAE_POOL_CLS_MEAN_PATCHES differs from MAE_POOL_MEAN_PATCHES")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid,pool", [("tap-s5D320-bf16-l2", CLS_MEAN), ("tap-s6D32-f32-none", CLS_MEAN), ("tap-s10D1024-f32-l2", MEAN_PATCHES)])
def test_image_does_not_depend_on_the_batch(dev, cid, pool):
    c, s = EXTRA[cid], stream(dev)
    t = {k: up(v, dev) for k, v in R.gen_pool(c).items()}
    W = 2 * c.D if pool == CLS_MEAN else c.D
    whole = torch.full((c.B, W), float("nan"), device=dev)
    tap(t["x"], t["branch"], c, t, c.B, c.seq, 1, pool, whole, W, s)
    for b in range(c.B):
        one = torch.full((2, W), float("nan"), device=dev)
        tap(t["x"][b], t["branch"][b], c, t, 1, c.seq, 1, pool, one, W, s)
        torch.cuda.synchronize()
        assert torch.equal(bits(one[0]), bits(whole[b])), f"image {b} alone differs from image {b} of {c.B}"
        assert torch.isnan(one[1]).all()


@pytest.mark.parametrize("shape", [(5, 8), (2, 1024)], ids=lambda g: "s{}D{}".format(*g))
def test_features_pool_takes_a_4_byte_aligned_out(dev, shape):
    """mae_features_pool's out may start at any float (the 16-byte rule is mae_features_tap's): one float into a NaN-filled buffer,
    at the narrowest and the widest row of the lane partition, it writes the aligned call's bits and nothing around them."""
    s = stream(dev)
    for c in (c for c in EXTRA.values() if (c.seq, c.D) == shape):
        t = {k: up(v, dev) for k, v in R.gen_pool(c).items()}
        for lo, hi in ((0, 1), (1, c.seq), (0, c.seq)):
            want = pool_out(c, t, lo, hi, s, dev)
            buf = torch.full((c.B * c.D + 8,), float("nan"), device=dev)
            assert buf.data_ptr() % 16 == 0
            check(lib.mae_features_pool(_ptr(t["x"]), _ptr(t["branch"]), DT[c.dtype], _ptr(t["gamma"]), _ptr(t["beta"]), R.EPS, c.B, c.seq, c.D, lo, hi,
                                        int(c.l2), _ptr(buf[1:]), s))
            torch.cuda.synchronize()
            assert torch.equal(bits(buf[1:1 + c.B * c.D]), bits(want).view(-1)), (c.id, lo, hi)
            assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + c.B * c.D:]).all(), (c.id, lo, hi)


def test_refused_call_writes_nothing(dev):
    c, s = EXTRA["tap-s5D8-f32-none"], stream(dev)
    t = {k: up(v, dev) for k, v in R.gen_pool(c).items()}
    buf = torch.full((c.B, 2 * c.D), float("nan"), device=dev)
    for kw, word in ((dict(with_cls=0, pool=CLS_MEAN), "with_cls"), (dict(with_cls=0, pool=CLS), "with_cls"), (dict(pool=4), "pool"),
                     (dict(stride=c.D - 4), "out_row_stride"), (dict(stride=2 * c.D - 4, pool=CLS_MEAN), "out_row_stride"), (dict(stride=c.D + 2), "out_row_stride"),
                     (dict(off=1), "aligned"), (dict(seq=1, pool=MEAN_PATCHES), "seq_len"), (dict(seq=1, pool=CLS_MEAN), "seq_len")):
        a = dict(with_cls=1, pool=MEAN, stride=2 * c.D, off=0, seq=c.seq)
        a.update(kw)
        rc = lib.mae_features_tap(_ptr(t["x"]), _ptr(t["branch"]), DT[c.dtype], _ptr(t["gamma"]), _ptr(t["beta"]), R.EPS, c.B, a["seq"], c.D, a["with_cls"],
                                  a["pool"], 0, _ptr(buf.view(-1)[a["off"]:]), a["stride"], s)
        check(0)
        assert rc != 0 and word in lib.mae_last_error().decode(), (kw, lib.mae_last_error())
    torch.cuda.synchronize()
    assert torch.isnan(buf).all()


def test_zz_print_worst_ratios():
    """Worst error / bound per variant over the tests above (bit-exact variants print 0)."""
    for k in sorted(WORST):
        print(f"features_tap.out  {k:28s} {WORST[k][0]:.3f}  ({WORST[k][1]})")
    assert all(np.isfinite(v[0]) and v[0] <= 1.0 for v in WORST.values())
