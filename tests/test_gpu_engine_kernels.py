"""The kernels only the engine launches -- full_grad_split / patch_grad_split, zero_token_rows (k_classifier.hip), features_pool
(k_representation.hip), cast, add_rows_pos, add_into (k_patch.hip) and linear_dgrad on the tiled fp32 kernel (k_gemm.hip) -- one by
one through their C entries against tests/engine_kernels_ref.py (-m gpu).

Every case of the reference's tables, on the reference's inputs.  Copies, bf16 roundings, zeros, single fp32 additions, the column
sums of the integer inputs and the pools of constant rows are compared bit for bit; dpos on random data, features_pool and
linear_dgrad inside bounds the reference's docstring counts from the code.  Every output buffer starts NaN-filled (or holds the
values the kernel must keep) with guard rows behind it and is compared as a whole; two launches into separate buffers must agree
bit for bit; a refused call must leave every buffer as it was.  linear_dgrad runs with fp32, bf16 -> bf16 and bf16 -> fp32
operands and outputs; of these the engine itself only uses fp32 (its bf16 dgrads are NT GEMMs on a transposed weight copy).  The
last test prints the worst error / bound per kernel and output.

The whole file (136 tests) takes about 2 s on an MI355X, 6 s with the start of the interpreter and the library
(profiles/r18_engine_kernel_ratios.txt); the largest buffers hold 17 MB."""
import pytest
import torch

from tests import engine_kernels_ref as R
from tests.test_gpu_token_kernels import rejected, run_twice, up
from tests.util import _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1}   # MAE_F32, MAE_BF16
U8 = 2                       # MAE_U8: no kernel here takes it
SPLIT = {c.id: c for c in R.split_cases()}
ZERO = {c.id: c for c in R.zero_cases()}
POOL = {c.id: c for c in R.pool_cases()}
ELEM = {c.id: c for c in R.elem_cases()}
POS = {c.id: c for c in R.pos_cases()}
GEMM = {c.id: c for c in R.gemm_cases()}
POOL_GROUPS = sorted({(c.D, c.seq, c.lo, c.hi) for c in POOL.values()})
GEMM_SHAPES = [f"{M}x{N}x{K}" for M, N, K in R.GEMM_SHAPES]
WORST = {}   # (kernel.output, variant) -> (worst error / bound, case id)


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def settle(cid, variant, e, got, init, fails_out, extra=()):
    ratios, fails = R.judge(e, got, init)
    for k, v in ratios.items():
        if (k, variant) not in WORST or v > WORST[(k, variant)][0]:
            WORST[(k, variant)] = (v, cid)
    print(cid, variant, {k: f"{v:.3f}" for k, v in ratios.items() if not isinstance(e[k], R.Exact)})
    fails_out += [f"{cid} [{variant}] {f}" for f in fails + list(extra)]


# ------------------------------------------------------------------------------------------------ full_grad_split
def split_call(c, dx, b, s, dtype=None, dim=None):
    return lib.mae_full_grad_split(_ptr(dx), c.B, c.L, c.D if dim is None else dim, int(c.with_cls), DT[c.dtype] if dtype is None else dtype,
                                   _ptr(b["full_grad_split.dtok"]), _ptr(b["full_grad_split.dpos"]), _ptr(b["full_grad_split.dcls"]),
                                   _ptr(b["full_grad_split.partial"]), s)


@pytest.mark.parametrize("cid", list(SPLIT))
def test_full_grad_split(dev, cid):
    c, s, fails = SPLIT[cid], stream(dev), []
    assert R.slices(c.B, c.L, c.D) == c.S and lib.mae_full_grad_split_partial_floats(c.B, c.L, c.D) == c.S * c.L * c.D
    for exact in (False, True):
        d = R.gen_split(c, exact)
        init, e, dx = R.split_inits(c), R.expect_split(c, d, exact), up(d["dx"], dev)
        got = run_twice(init, lambda b: check(split_call(c, dx, b, s)), dev, cid)
        settle(cid, ("cls " if c.with_cls else "patch ") + c.dtype + (" integers" if exact else ""), e, got, init, fails, R.split_extra(c, got))
    assert not fails, "\n".join(fails)


def test_full_grad_split_refuses_before_it_launches(dev):
    s = stream(dev)
    for cid in ("B3L5D8-cls-f32", "B3L5D8-patch-bf16"):
        c = SPLIT[cid]
        init, dx = R.split_inits(c), up(R.gen_split(c)["dx"], dev)
        for kw, message in ((dict(dtype=U8), "dtype must be MAE_F32 or MAE_BF16"), (dict(dtype=-1), "dtype must be"), (dict(dim=0), "multiple of 4 in [4, 1024]"),
                            (dict(dim=6), "multiple of 4 in [4, 1024]"), (dict(dim=1028), "multiple of 4 in [4, 1024]")):
            assert rejected(lambda b: split_call(c, dx, b, s, **kw), init, message, dev), (cid, kw)
    for args in ((0, 5, 8), (3, 0, 8), (3, 5, 0), (3, 5, 2), (3, 5, 1028), (1 << 20, 1 << 11, 8)):
        assert lib.mae_full_grad_split_partial_floats(*args) == -1, args


# ------------------------------------------------------------------------------------------------ zero_token_rows
def zero_call(c, b, s, dtype=None, dim=None):
    return lib.mae_zero_token_rows(c.rows, c.L, c.D if dim is None else dim, DT[c.dtype] if dtype is None else dtype, _ptr(b["zero_token_rows.dres"]),
                                   _ptr(b["zero_token_rows.dres_c"]), s)


@pytest.mark.parametrize("cid", list(ZERO))
def test_zero_token_rows(dev, cid):
    c, s, fails = ZERO[cid], stream(dev), []
    d = R.gen_zero(c)
    init, e = R.zero_inits(c, d), R.expect_zero(c, d)
    settle(cid, c.dtype, e, run_twice(init, lambda b: check(zero_call(c, b, s)), dev, cid), init, fails)
    assert not fails, "\n".join(fails)


def test_zero_token_rows_refuses_before_it_launches(dev):
    c, s = ZERO["D8-L5-bf16"], stream(dev)
    init = R.zero_inits(c, R.gen_zero(c))
    for kw, message in ((dict(dim=0), "multiple of 4 in [4, 1024]"), (dict(dim=2), "multiple of 4 in [4, 1024]"), (dict(dim=1028), "multiple of 4 in [4, 1024]"),
                        (dict(dtype=U8), "dtype must be MAE_F32 or MAE_BF16")):
        assert rejected(lambda b: zero_call(c, b, s, **kw), init, message, dev), kw


# ------------------------------------------------------------------------------------------------ features_pool
def pool_call(c, t, out, s, B=None, **kw):
    a = dict(dtype=DT[c.dtype], dim=c.D, lo=c.lo, hi=c.hi, normalize=int(c.l2))
    a.update(kw)
    return lib.mae_features_pool(_ptr(t["x"]), _ptr(t["branch"]), a["dtype"], _ptr(t["gamma"]), _ptr(t["beta"]), R.EPS, c.B if B is None else B, c.seq, a["dim"],
                                 a["lo"], a["hi"], a["normalize"], _ptr(out), s)


@pytest.mark.parametrize("group", POOL_GROUPS, ids=lambda g: "D{}-s{}r{}_{}".format(*g))
def test_features_pool(dev, group):
    s, fails = stream(dev), []
    for c in (c for c in POOL.values() if (c.D, c.seq, c.lo, c.hi) == group):
        d = R.gen_pool(c)
        init, e = R.pool_inits(c), R.expect_pool(c, d)
        t = {k: up(v, dev) for k, v in d.items()}
        got = run_twice(init, lambda b: check(pool_call(c, t, b["features_pool.out"], s)), dev, c.id)
        settle(c.id, f"{c.kind} {c.dtype} {'l2' if c.l2 else 'none'}", e, got, init, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", ["D260-s10r1_10-bf16-l2", "D8-s10r1_4-f32-none", "D1024-s10r0_10-f32-l2"])
def test_features_pool_image_does_not_depend_on_the_batch(dev, cid):
    c, s = POOL[cid], stream(dev)
    d = R.gen_pool(c)
    t = {k: up(v, dev) for k, v in d.items()}
    whole = up(R.pool_inits(c)["features_pool.out"], dev)
    check(pool_call(c, t, whole, s))
    for b in range(c.B):
        one = up(R.nan_buf(1, c.D), dev)
        alone = dict(t, x=t["x"][b:b + 1].contiguous(), branch=t["branch"][b:b + 1].contiguous())    # held until the synchronize below
        check(pool_call(c, alone, one, s, B=1))
        torch.cuda.synchronize()
        assert torch.equal(one[:1].view(torch.int32), whole[b:b + 1].view(torch.int32)), f"image {b} alone differs from image {b} of {c.B}"
        assert torch.isnan(one[1:]).all()


def test_features_pool_refuses_before_it_launches(dev):
    c, s = POOL["D8-s10r1_4-f32-none"], stream(dev)
    t = {k: up(v, dev) for k, v in R.gen_pool(c).items()}
    init = R.pool_inits(c)
    for kw, message in ((dict(dtype=U8), "branch dtype must be MAE_F32 or MAE_BF16"), (dict(dim=0), "multiple of 4 in [4, 1024]"), (dict(dim=6), "multiple of 4 in [4, 1024]"),
                        (dict(lo=4), "outside the sequence"), (dict(hi=c.seq + 1), "outside the sequence"), (dict(lo=-1), "outside the sequence"),
                        (dict(normalize=2), "normalize must be MAE_FEAT_NONE or MAE_FEAT_L2")):
        assert rejected(lambda b: pool_call(c, t, b["features_pool.out"], s, **kw), init, message, dev), kw


# ------------------------------------------------------------------------------------------------ cast, add_into, add_rows_pos
@pytest.mark.parametrize("cid", list(ELEM))
def test_cast(dev, cid):
    c, s, fails = ELEM[cid], stream(dev), []
    for src, dst in R.DT_PAIRS:
        d = R.gen_cast(c, src)
        init, e, x = R.cast_inits(c, dst), R.expect_cast(c, d, src, dst), up(d["src"], dev)
        got = run_twice(init, lambda b: check(lib.mae_cast(_ptr(x), DT[src], _ptr(b["cast.dst"]), DT[dst], c.n, s)), dev, cid)
        settle(cid, f"{src} -> {dst}", e, got, init, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", list(ELEM))
def test_add_into(dev, cid):
    c, s, fails = ELEM[cid], stream(dev), []
    for dt in ("f32", "bf16"):
        d = R.gen_add_into(c, dt)
        init, e, src = R.add_into_inits(c, d), R.expect_add_into(c, d), up(d["src"], dev)
        got = run_twice(init, lambda b: check(lib.mae_add_into(_ptr(src), _ptr(b["add_into.dst"]), DT[dt], c.n, s)), dev, cid)
        settle(cid, dt, e, got, init, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", list(POS))
def test_add_rows_pos(dev, cid):
    c, s, fails = POS[cid], stream(dev), []
    d = R.gen_pos(c)
    init, e, x, pos = R.pos_inits(c), R.expect_pos(c, d), up(d["x"], dev), up(d["pos"], dev)
    got = run_twice(init, lambda b: check(lib.mae_add_rows_pos(_ptr(x), _ptr(pos), c.rows, c.L, c.D, _ptr(b["add_rows_pos.out"]), s)), dev, cid)
    settle(cid, "", e, got, init, fails)
    assert not fails, "\n".join(fails)


def test_element_kernels_refuse_before_they_launch(dev):
    """launch_cast used to send any dtype pair it did not know to the bf16 -> bf16 kernel."""
    c, s = ELEM["n257"], stream(dev)
    x = up(R.gen_cast(c, "f32")["src"], dev)
    for src, dst in ((U8, 0), (0, U8), (U8, U8), (1, U8), (-1, 1), (3, 3)):
        assert rejected(lambda b: lib.mae_cast(_ptr(x), src, _ptr(b["cast.dst"]), dst, c.n, s), R.cast_inits(c, "f32"), "cast: dtypes must be MAE_F32 or MAE_BF16", dev), (src, dst)
    assert rejected(lambda b: lib.mae_cast(_ptr(x), 0, _ptr(b["cast.dst"]), 1, 0, s), R.cast_inits(c, "bf16"), "cast: bad arguments", dev)
    d = R.gen_add_into(c, "f32")
    src = up(d["src"], dev)
    assert rejected(lambda b: lib.mae_add_into(_ptr(src), _ptr(b["add_into.dst"]), U8, c.n, s), R.add_into_inits(c, d), "add_into: dtype must be MAE_F32 or MAE_BF16", dev)
    p = POS["r7L3D4"]
    dp = R.gen_pos(p)
    xp, pos = up(dp["x"], dev), up(dp["pos"], dev)
    for dim in (0, 2, 6):
        assert rejected(lambda b: lib.mae_add_rows_pos(_ptr(xp), _ptr(pos), p.rows, p.L, dim, _ptr(b["add_rows_pos.out"]), s), R.pos_inits(p),
                        "positive multiple of 4", dev), dim


# ------------------------------------------------------------------------------------------------ linear_dgrad
def gemm_call(c, t, b, s, **kw):
    a = dict(dtype=DT[c.dtype], mode=c.mode, out=DT[c.out])
    a.update(kw)
    return lib.mae_linear_dgrad(_ptr(t["dy"]), _ptr(t["w"]), c.M, c.N, c.K, a["dtype"], a["mode"], a["out"], _ptr(b["linear_dgrad.out"]), _ptr(t["aux"]), s)


@pytest.mark.parametrize("shape", GEMM_SHAPES)
def test_linear_dgrad(dev, shape):
    """fp32 operands are what the engine launches; the bf16 instantiations exist in the library and are checked with it."""
    s, fails = stream(dev), []
    for c in (c for c in GEMM.values() if c.id.startswith(shape + "-")):
        d = R.gen_gemm(c)
        init, e = R.gemm_inits(c), R.expect_gemm(c, d)
        t = {k: up(v, dev) for k, v in d.items()}
        got = run_twice(init, lambda b: check(gemm_call(c, t, b, s)), dev, c.id)
        settle(c.id, f"{R.MODE_NAME[c.mode]} {c.dtype} -> {c.out}", e, got, init, fails)
    assert not fails, "\n".join(fails)


def test_linear_dgrad_refuses_before_it_launches(dev):
    c, s = GEMM["31x20x24-mul-bf16-bf16"], stream(dev)
    t = {k: up(v, dev) for k, v in R.gen_gemm(c).items()}
    init = R.gemm_inits(c)
    for kw, message in ((dict(dtype=U8), "bad dtype 2"), (dict(out=U8), "bad output dtype 2"), (dict(dtype=0, out=1), "fp32 operands with bf16 output"),
                        (dict(mode=1), "GELU epilogue needs out2"), (dict(mode=2), "RESID epilogue writes fp32"), (dict(mode=6), "epilogue must be NONE, DGELU or MUL"),
                        (dict(mode=9), "unknown epilogue")):
        assert rejected(lambda b: gemm_call(c, t, b, s, **kw), init, message, dev), kw


def test_zz_report():
    """Prints the worst error / bound per kernel output and variant over the cases that ran (0 = bit-exact everywhere)."""
    print("\nworst error / bound per output and variant:")
    for (k, variant), (ratio, cid) in sorted(WORST.items()):
        print(f"  {k:40s} {variant:24s} {ratio:.3f}  ({cid})")
    assert WORST and all(v[0] <= 1.0 for v in WORST.values())
    assert {k.split(".")[0] for k, _ in WORST} == set(R.KERNELS)
