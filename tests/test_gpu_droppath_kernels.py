"""The per-image branch scale of the LayerNorm kernels (drop path; k_layernorm.hip) through mae_add_layernorm_fwd_scaled and
mae_layernorm_bwd_scaled, per element (-m gpu).

Shapes: the eight selectable (lanes per row, vectors per lane) pairs of ln_ref.PAIRS at their smallest and largest dim, fp32 and
bf16, over 7 images of 5 rows (35 rows: lane groups without a row, and rows of one wave that belong to two images); one grid-stride
second-trip case each way at dim 8 with 4 rows per image; one row-mapped case whose map is the class rows b * T.  The backward runs
with accumulate 0 and 1.  Outputs are NaN-filled with guard rows behind them, two launches must agree bit for bit and rows outside
the map stay untouched.

Forward.  Scale 1 everywhere equals mae_add_layernorm_fwd in every bit.  A scale of 0 leaves x_out = x in every bit although the
branch rows of those images hold NaN.  On grid data (x multiples of 2^-12 in [-8, 8], branch multiples of 2^-6 in [-4, 4], scales
multiples of 2^-10 in [0, 2]) s * b and x + s * b are exact in fp32 with or without a fused multiply-add, so x_out equals the
float64 value bit for bit.  On general data |x_out - (x + s b)| <= u (|s b| + |x + s b|), u = 2^-24: one rounding of the product, one
of the sum (a fused multiply-add only removes the first).  y, mean and rstd are judged by ln_ref's forward bounds on the x_out the
device wrote, with no branch: the LayerNorm is taken of the stored sum.

Backward.  dx_io, dgamma and dbeta equal mae_layernorm_bwd's in every bit; dx_copy equals T(fl32(fl32(s) * dx_io)) formed on the
host from the device's dx_io (one fp32 product, then tests.optim_ref.bf16_rne for bf16), signed zeros compared as numbers; a NULL
scale vector equals the old call in every bit."""
from dataclasses import dataclass

import numpy as np
import pytest
import torch

from tests import ln_ref as R
from tests.test_gpu_layernorm import GUARD_ROWS, Out, put
from tests.util import BF16, F32, TDT, _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24
SCALES = np.array([0.0, 1.0, 2.0, F(1.0 / 0.9), 0.37, 0.0, 1.0], dtype=F)             # per image, cycled
GRID_SCALES = np.array([0.0, 1.0, 2.0, 1138 / 1024, 379 / 1024, 1 / 1024, 2047 / 1024], dtype=F)   # multiples of 2^-10


@dataclass(frozen=True)
class Case:
    dtype: str
    images: int
    T: int            # rows per image
    dim: int
    cls_map: bool     # the row map b * T: one row per image
    kind: str         # "table" | "fwd_wrap" | "bwd_wrap" | "map"

    @property
    def src_rows(self):
        return self.images * self.T

    @property
    def rows(self):
        return self.images if self.cls_map else self.src_rows

    @property
    def id(self):
        return f"{self.dtype}-{self.images}x{self.T}x{self.dim}-{self.kind}"


def cases():
    out = []
    for dtype in ("fp32", "bf16"):
        for _lpr, _nv, lo, hi in R.PAIRS:
            out += [Case(dtype, 7, 5, lo, False, "table"), Case(dtype, 7, 5, hi, False, "table")]
        out.append(Case(dtype, (8192 * 16 + 20) // 4, 4, 8, False, "fwd_wrap"))
        out.append(Case(dtype, (1024 * 16 + 20) // 4, 4, 8, False, "bwd_wrap"))
        out.append(Case(dtype, 7, 5, 192, True, "map"))
    return out


CASES = cases()
BY_ID = {c.id: c for c in CASES}
FWD = [c.id for c in CASES if c.kind != "bwd_wrap"]
BWD = [c.id for c in CASES if c.kind != "fwd_wrap"]


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def _dt(c):
    return BF16 if c.dtype == "bf16" else F32


def _rng(c, salt):
    return np.random.default_rng(R._seed(c, salt))


def _map(c):
    return (np.arange(c.images) * c.T).astype(np.int32) if c.cls_map else None


def _image_scales(c, table):
    return table[np.arange(c.images) % len(table)].astype(F)


def test_case_table_covers_the_issue():
    for dtype in ("fp32", "bf16"):
        mine = [c for c in CASES if c.dtype == dtype]
        for lpr, nv, lo, hi in R.PAIRS:
            for dim in (lo, hi):
                g = R.geometry(35, dim)
                assert (g.lpr, g.nv) == (lpr, nv) and any(c.dim == dim and c.rows == 35 for c in mine)
        assert R.geometry(16, 4).rpw == 4 and 35 % 4 != 0 and 5 % 4 != 0     # lane groups without a row; a wave's rows straddle two images
        fw = [c for c in mine if c.kind == "fwd_wrap"][0]
        bw = [c for c in mine if c.kind == "bwd_wrap"][0]
        assert fw.rows == 8192 * 16 + 20 and fw.rows % fw.T == 0 and R.geometry(fw.rows, fw.dim).fwd_trips == 2
        assert bw.rows == 1024 * 16 + 20 and bw.rows % bw.T == 0 and R.geometry(bw.rows, bw.dim).bwd_trips == 2
        assert any(c.cls_map for c in mine)
    assert set(SCALES.tolist()) == {0.0, 1.0, 2.0, float(F(1.0 / 0.9)), float(F(0.37))}
    assert np.array_equal(GRID_SCALES * 1024, np.round(GRID_SCALES * 1024)) and GRID_SCALES.max() <= 2


# ------------------------------------------------------------------------------------------------ forward
def fwd_launch(c, dev, x, branch, gamma, beta, scale, scaled=True):
    """Two launches into separate NaN-filled, guarded outputs, compared bit for bit -> dict of Out (the first launch's)."""
    dt, tdt = _dt(c), TDT[_dt(c)]
    xd, bd, gd, be = put(x, dev), put(branch, dev, tdt), put(gamma, dev), put(beta, dev)
    rmap, sd = put(_map(c), dev, torch.int32), put(scale, dev)
    sets = []
    for _ in range(2):
        o = dict(y=Out(c.rows, c.dim, tdt, dev), mean=Out(c.rows, 0, torch.float32, dev), rstd=Out(c.rows, 0, torch.float32, dev),
                 x_out=Out(c.src_rows, c.dim, torch.float32, dev))
        head = (_ptr(xd), _ptr(bd), _ptr(o["x_out"].full), _ptr(rmap), _ptr(gd), _ptr(be), R.EPS, c.rows, c.dim, dt, _ptr(o["y"].full),
                _ptr(o["mean"].full), _ptr(o["rstd"].full))
        if scaled:
            check(lib.mae_add_layernorm_fwd_scaled(*head, _ptr(sd), c.T, stream(dev)))
        else:
            check(lib.mae_add_layernorm_fwd(*head, stream(dev)))
        sets.append(o)
    torch.cuda.synchronize()
    for k in sets[0]:
        assert sets[0][k].guard_intact() and sets[1][k].guard_intact(), f"{c.id}: guard rows of {k} were written"
        assert torch.equal(sets[0][k].bits(), sets[1][k].bits()), f"{c.id}: two launches differ in {k}"
    return sets[0]


def _src(c):
    return R._src(c.rows, _map(c))


def _untouched(c, o):
    rest = R._outside(c.src_rows, _src(c))
    assert np.isnan(o["x_out"].host()[rest]).all(), f"{c.id}: x_out rows outside the map were written"


@pytest.mark.parametrize("cid", FWD)
def test_forward_scaled_per_element(dev, cid):
    c = BY_ID[cid]
    r = _rng(c, 11)
    n, dim, src = c.src_rows, c.dim, _src(c)
    s_img = _image_scales(c, SCALES)
    s_row = s_img[np.arange(n) // c.T]
    x = (r.standard_normal((n, dim)) * 2.0 + 0.3).astype(F)
    branch = R._round(r.standard_normal((n, dim)) * 0.5, c.dtype)
    gamma, beta = r.standard_normal(dim).astype(F), r.standard_normal(dim).astype(F)
    poisoned = branch.copy()
    poisoned[s_row == 0] = np.nan                      # a dropped image's branch is never read
    o = fwd_launch(c, dev, x, poisoned, gamma, beta, s_img)
    _untouched(c, o)
    xo, y, mean, rstd = o["x_out"].host()[src], o["y"].host(), o["mean"].host(), o["rstd"].host()
    assert all(np.isfinite(a).all() for a in (xo, y, mean, rstd)), f"{cid}: an output is not finite"
    dropped = s_row[src] == 0
    assert dropped.any() and np.array_equal(R._bits(xo[dropped]), R._bits(x[src][dropped])), f"{cid}: a dropped row's x_out is not x bit for bit"
    # the scaled sum: one rounding of the product, one of the sum
    sb = R._d(s_row[src])[:, None] * R._d(branch[src])
    want = R._d(x[src]) + sb
    ratio, i = R.worst(xo, want, U * (np.abs(sb) + np.abs(want)))
    print(cid, f"x_out error / bound {ratio:.3f}")
    assert ratio <= 1.0, f"{cid}: x_out error / bound {ratio:.3g} at {R.locate(R.geometry(c.rows, dim), *divmod(i, dim), False)}"
    # the LayerNorm of the stored sum
    full = o["x_out"].host()
    full[R._outside(n, src)] = 0.0
    ref = R.fwd_ref(full, gamma, beta, c.rows, _map(c))
    b = R.fwd_bounds(ref, R.geometry(c.rows, dim), gamma, beta, c.dtype == "bf16")
    for name, got in (("mean", mean), ("rstd", rstd), ("y", y)):
        ratio, i = R.worst(got, ref[name], b[name])
        assert ratio <= 1.0, f"{cid}: {name} error / bound {ratio:.3g} (flat index {i})"


@pytest.mark.parametrize("cid", FWD)
def test_forward_scale_one_is_the_unscaled_call_and_grid_data_is_exact(dev, cid):
    c = BY_ID[cid]
    r = _rng(c, 12)
    n, dim, src = c.src_rows, c.dim, _src(c)
    gamma, beta = r.standard_normal(dim).astype(F), r.standard_normal(dim).astype(F)
    x = (r.standard_normal((n, dim)) * 2.0 + 0.3).astype(F)
    branch = R._round(r.standard_normal((n, dim)) * 0.5, c.dtype)
    a = fwd_launch(c, dev, x, branch, gamma, beta, np.ones(c.images, F))
    b = fwd_launch(c, dev, x, branch, gamma, beta, None, scaled=False)
    for k in a:
        assert torch.equal(a[k].bits(), b[k].bits()), f"{cid}: scale 1 differs from mae_add_layernorm_fwd in {k}"
    # grid data: every intermediate is exact, contracted or not
    x = (r.integers(-8 * 4096, 8 * 4096 + 1, (n, dim)) / 4096.0).astype(F)
    branch = (r.integers(-4 * 64, 4 * 64 + 1, (n, dim)) / 64.0).astype(F)
    assert np.array_equal(R._round(branch, c.dtype), branch)
    s_img = _image_scales(c, GRID_SCALES)
    s_row = s_img[np.arange(n) // c.T]
    o = fwd_launch(c, dev, x, branch, gamma, beta, s_img)
    _untouched(c, o)
    want = R._d(x[src]) + R._d(s_row[src])[:, None] * R._d(branch[src])
    assert np.array_equal(want.astype(F).astype(np.float64), want)        # representable: the float64 value is the fp32 value
    bad = np.argwhere(R._bits(o["x_out"].host()[src]) != R._bits(want.astype(F)))
    assert not bad.size, f"{cid}: x_out differs from the exact x + s * branch in {len(bad)} elements, first at row {bad[0][0]} col {bad[0][1]}"


# ------------------------------------------------------------------------------------------------ backward
def bwd_launch(c, dev, d, accumulate, scale, scaled=True):
    dt, tdt = _dt(c), TDT[_dt(c)]
    x, gamma, dy = put(d["x"], dev), put(d["gamma"], dev), put(d["dy"], dev, tdt)
    mu, rs, rmap, sd = put(d["mean"], dev), put(d["rstd"], dev), put(_map(c), dev, torch.int32), put(scale, dev)
    sets = []
    for _ in range(2):
        o = dict(dx=Out(c.src_rows, c.dim, torch.float32, dev, d["res"] if accumulate else None), dx_copy=Out(c.src_rows, c.dim, tdt, dev),
                 dgamma=Out(c.dim, 0, torch.float32, dev), dbeta=Out(c.dim, 0, torch.float32, dev),
                 partial=Out(2 * R.LN_BWD_MAX_BLOCKS * c.dim, 0, torch.float32, dev))
        head = (_ptr(dy), dt, _ptr(x), _ptr(rmap), _ptr(gamma), _ptr(mu), _ptr(rs), c.rows, c.dim, accumulate, _ptr(o["dx"].full),
                _ptr(o["dx_copy"].full), _ptr(o["dgamma"].full), _ptr(o["dbeta"].full), _ptr(o["partial"].full))
        if scaled:
            check(lib.mae_layernorm_bwd_scaled(*head, _ptr(sd), c.T, stream(dev)))
        else:
            check(lib.mae_layernorm_bwd(*head, stream(dev)))
        sets.append(o)
    torch.cuda.synchronize()
    for k in sets[0]:
        assert sets[0][k].guard_intact() and sets[1][k].guard_intact(), f"{c.id}: guard rows of {k} were written"
        assert torch.equal(sets[0][k].bits(), sets[1][k].bits()), f"{c.id}: two launches differ in {k}"
    return sets[0]


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("cid", BWD)
def test_backward_scaled_copy(dev, cid, accumulate):
    c = BY_ID[cid]
    r = _rng(c, 13)
    n, dim, src = c.src_rows, c.dim, _src(c)
    x = (r.standard_normal((n, dim)) * 2.0 + 0.3).astype(F)
    gamma = r.standard_normal(dim).astype(F)
    st = R.fwd_ref(x, gamma, np.zeros(dim, F), c.rows, _map(c))
    d = dict(x=x, gamma=gamma, dy=R._round(r.standard_normal((c.rows, dim)), c.dtype), res=r.standard_normal((n, dim)).astype(F),
             mean=st["mean"].astype(F), rstd=st["rstd"].astype(F))
    s_img = _image_scales(c, SCALES)
    s_row = s_img[np.arange(n) // c.T]
    old = bwd_launch(c, dev, d, accumulate, None, scaled=False)
    new = bwd_launch(c, dev, d, accumulate, s_img)
    null = bwd_launch(c, dev, d, accumulate, None)
    for k in ("dx", "dgamma", "dbeta"):
        assert torch.equal(new[k].bits(), old[k].bits()), f"{cid}: {k} differs from mae_layernorm_bwd"
    for k in old:
        if k != "partial":
            assert torch.equal(null[k].bits(), old[k].bits()), f"{cid}: a NULL scale differs from mae_layernorm_bwd in {k}"
    dx = new["dx"].host()
    assert np.isfinite(dx[src]).all()
    prod = s_row[src][:, None].astype(F) * dx[src].astype(F)          # one fp32 product of the value the device stored
    assert prod.dtype == F
    want = R.to_bf16(prod) if c.dtype == "bf16" else prod
    got = new["dx_copy"].host()
    bad = np.argwhere(got[src] != want)                                # signed zeros compare as numbers
    assert not bad.size, (f"{cid}: dx_copy differs from T(fl32(s * dx_io)) in {len(bad)} elements, first row {bad[0][0]} col {bad[0][1]}: "
                          f"got {got[src][tuple(bad[0])]!r} want {want[tuple(bad[0])]!r}")
    rest = R._outside(n, src)
    assert np.isnan(got[rest]).all(), f"{cid}: dx_copy rows outside the map were written"
    init = d["res"] if accumulate else np.full((n, dim), np.nan, F)
    assert np.array_equal(R._bits(dx[rest]), R._bits(init[rest])), f"{cid}: dx rows outside the map were written"
    assert (got[src][s_row[src] == 0] == 0).all() and (s_row[src] == 0).any()


def test_scaled_calls_refuse_rows_per_image_below_one(dev):
    c = BY_ID["fp32-7x5x64-table"]
    t = torch.zeros(c.src_rows + GUARD_ROWS, c.dim, device=dev)
    v = torch.ones(2 * R.LN_BWD_MAX_BLOCKS * c.dim, device=dev)
    for rpi in (0, -5):
        rc = lib.mae_add_layernorm_fwd_scaled(_ptr(t), _ptr(t), _ptr(t), None, _ptr(v), _ptr(v), R.EPS, c.rows, c.dim, F32, _ptr(t), _ptr(v), _ptr(v),
                                              _ptr(v), rpi, stream(dev))
        assert rc != 0 and b"rows_per_image" in lib.mae_last_error()
        rc = lib.mae_layernorm_bwd_scaled(_ptr(t), F32, _ptr(t), None, _ptr(v), _ptr(v), _ptr(v), c.rows, c.dim, 0, _ptr(t), _ptr(t), _ptr(v), _ptr(v),
                                          _ptr(v), _ptr(v), rpi, stream(dev))
        assert rc != 0 and b"rows_per_image" in lib.mae_last_error()
    check(0)
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0      # refused before any launch
