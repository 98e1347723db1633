"""tests/engine_kernels_ref.py on the CPU: the case tables reach every path the kernels have; the plain fp32 evaluation in the
kernel's own order stays inside the reference's bounds and exactness claims for every case (the condition on the inputs); the
reference agrees with independent float64 code; and every mutant -- a slice boundary off by one image, a dropped u tail, a copied
class row, dcls from row 1, r % (L + 1), a skipped last grid trip or lane pass, the divisor seq_len, a skipped column, a wave
short, truncation instead of rounding, a reduction cut at a multiple of 16, a missing last column, a transposed side input, one
bf16 / fp32 ulp, a written guard row -- fails."""
import math

import numpy as np
import pytest
import torch

from tests import engine_kernels_ref as R

SPLIT = {c.id: c for c in R.split_cases()}
ZERO = {c.id: c for c in R.zero_cases()}
POOL = {c.id: c for c in R.pool_cases()}
ELEM = {c.id: c for c in R.elem_cases()}
POS = {c.id: c for c in R.pos_cases()}
GEMM = {c.id: c for c in R.gemm_cases()}


def passes(e, got, init, extra=()):
    ratios, fails = R.judge(e, got, init)
    fails = fails + list(extra)
    assert all(v <= 1.0 for v in ratios.values()) == (not [f for f in fails if f not in extra])
    return not fails


# ------------------------------------------------------------------------------------------------ the tables
def test_case_table_is_complete():
    assert R.coverage_gaps() == []
    for table in (SPLIT, ZERO, POOL, ELEM, POS, GEMM):
        assert len(table) > 2                                             # ids are unique: the dicts lost nothing
    assert len(SPLIT) == len(R.split_cases()) and len(POOL) == len(R.pool_cases()) and len(GEMM) == len(R.gemm_cases())


def test_a_thinned_table_has_gaps(monkeypatch):
    """coverage_gaps notices what it is there to notice."""
    full = R.split_cases()
    monkeypatch.setattr(R, "split_cases", lambda: [c for c in full if c.B != 60])
    assert any("block limit" in g for g in R.coverage_gaps())
    monkeypatch.setattr(R, "split_cases", lambda: [R.SplitCase(c.id, c.B, c.L, c.D, c.S + (c.B == 67), c.with_cls, c.dtype) for c in full])
    assert any("meant to reach 65" in g for g in R.coverage_gaps())
    monkeypatch.setattr(R, "split_cases", lambda: full)
    ranges = R.POOL_RANGES
    monkeypatch.setattr(R, "POOL_RANGES", tuple(r for r in ranges if r[2] - r[1] != 5))
    assert any("row counts" in g for g in R.coverage_gaps())


def test_slices_restate_the_launcher():
    """full_grad_split_slices by hand at the shapes of the table: per_slice blocks, then min(B, 64, ceil(2048 / per_slice))."""
    assert [R.slices(B, L, D) for B, L, D, _ in R.SPLIT_SHAPES] == [1, 3, 5, 64, 64, 54, 9] == [S for *_, S in R.SPLIT_SHAPES]
    assert math.ceil(50 * 192 / 256) == 38 and math.ceil(2048 / 38) == 54 and math.ceil(145 * 96 / 256) == 55
    assert sorted({b1 - b0 for b0, b1 in R.slice_bounds(300, 64)}) == [4, 5] and sorted({b1 - b0 for b0, b1 in R.slice_bounds(67, 64)}) == [1, 2]
    assert R.slice_bounds(67, 64)[0] == (0, 1) and R.slice_bounds(67, 64)[-1] == (65, 67) and 17 * 48 == 816


# ------------------------------------------------------------------------------------------------ simulate inside expect
@pytest.mark.parametrize("cid", list(SPLIT))
def test_split_simulation_passes(cid):
    c = SPLIT[cid]
    for exact in (False, True):
        d = R.gen_split(c, exact)
        got = R.simulate_split(c, d)
        assert passes(R.expect_split(c, d, exact), got, R.split_inits(c), R.split_extra(c, got)), (cid, exact)


def test_integer_sums_do_not_depend_on_the_order():
    c = SPLIT["B300L3D1024-cls-f32"]
    dx = R.gen_split(c, True)["dx"]
    ref = dx.astype(np.float64).sum(0)
    for s in (np.add.accumulate(dx, axis=0, dtype=np.float32)[-1], np.add.accumulate(dx[::-1], axis=0, dtype=np.float32)[-1], dx.sum(0, dtype=np.float32)):
        assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), ref)
    assert all(np.abs(R.gen_split(k, True)["dx"]).astype(np.float64).sum(0).max() < 2 ** 24 for k in SPLIT.values())


@pytest.mark.parametrize("cid", list(ZERO))
def test_zero_simulation_passes(cid):
    c = ZERO[cid]
    d = R.gen_zero(c)
    init = R.zero_inits(c, d)
    got = R.simulate_zero(c, d)
    assert passes(R.expect_zero(c, d), got, init)
    if c.L == 1:
        assert all(np.array_equal(R.bits(got[k]), R.bits(init[k])) for k in init)       # nothing may change


@pytest.mark.parametrize("cid", list(POOL))
def test_pool_simulation_passes(cid):
    c = POOL[cid]
    d = R.gen_pool(c)
    assert np.isnan(d["x"]).sum() == c.B * (c.seq - c.n) * c.D
    assert passes(R.expect_pool(c, d), R.simulate_pool(c, d), R.pool_inits(c))


@pytest.mark.parametrize("cid", ["D260-s10r1_10-bf16-l2", "D8-s10r0_10-f32-none", "D1024-s10r2_6-f32-l2"])
def test_pool_reference_matches_torch(cid):
    """The float64 reference against torch's layer_norm in float64 on the fp32-rounded sum."""
    c = POOL[cid]
    d = R.gen_pool(c)
    v = torch.from_numpy((d["x"][:, c.lo:c.hi] + R.widen(d["branch"])[:, c.lo:c.hi]).astype(np.float32)).double()
    y = torch.nn.functional.layer_norm(v, (c.D,), torch.from_numpy(d["gamma"]).double(), torch.from_numpy(d["beta"]).double(), float(np.float32(R.EPS)))
    f = y.mean(1)
    if c.l2:
        f = f / (f.norm(dim=1, keepdim=True) + float(np.float32(1e-8)))
    e = R.expect_pool(c, d)["features_pool.out"]
    assert np.abs(e.ref - f.numpy()).max() < 1e-12 and (e.bound > 0).all() and e.bound.max() < 1e-4


@pytest.mark.parametrize("cid", list(ELEM))
def test_cast_and_add_into_simulations_pass(cid):
    c = ELEM[cid]
    for src, dst in R.DT_PAIRS:
        d = R.gen_cast(c, src)
        assert passes(R.expect_cast(c, d, src, dst), R.simulate_cast(c, d, src, dst), R.cast_inits(c, dst))
    for dt in ("f32", "bf16"):
        d = R.gen_add_into(c, dt)
        assert passes(R.expect_add_into(c, d), R.simulate_add_into(c, d), R.add_into_inits(c, d))


def test_cast_reference_matches_torch():
    """bf16_rne on the special patterns against torch's own fp32 -> bf16 conversion, and the widening back; the patterns are what the
    docstring says they are."""
    x = R.CAST_F32.view(np.float32).copy()
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne(x)
    fin = ~np.isnan(x)
    assert np.array_equal(got[fin], want[fin]) and ((got[~fin] & 0x7FC0) == 0x7FC0).all() and np.array_equal(got[~fin], (R.CAST_F32[~fin] >> 16) | 0x40)
    assert np.array_equal(R.widen(R.CAST_BF16).view(np.uint32), R.CAST_BF16.astype(np.uint32) << 16)
    as16 = dict(zip(R.CAST_F32.tolist(), got.tolist()))
    assert as16[0x3F808000] == 0x3F80 and as16[0x3F818000] == 0x3F82 and as16[0x3F808001] == 0x3F81 and as16[0x3F817FFF] == 0x3F81   # ties and their neighbours
    assert as16[0x7F7FFFFF] == 0x7F80 and as16[0x00000001] == 0 and as16[0x807FFFFF] == 0x8080 and as16[0x00018000] == 2 and as16[0x00008000] == 0
    d = R.gen_add_into(ELEM["n257"], "bf16")
    s = (R.widen(d["dst"]) + d["src"])[:4]
    assert ((s.view(np.uint32) & 0xFFFF) == 0x8000).all()                                 # the first four sums are bf16 ties
    assert R.expect_add_into(ELEM["n257"], d)["add_into.dst"].want[:4].tolist() == [0x3F82, 0x3F80, 0xBF82, 0xBF80]


@pytest.mark.parametrize("cid", list(POS))
def test_pos_simulation_passes(cid):
    c = POS[cid]
    d = R.gen_pos(c)
    e = R.expect_pos(c, d)
    assert passes(e, R.simulate_pos(c, d), R.pos_inits(c))
    want = torch.from_numpy(d["x"]) + torch.from_numpy(d["pos"])[torch.arange(c.rows) % c.L]
    assert np.array_equal(e["add_rows_pos.out"].want, want.numpy())


@pytest.mark.parametrize("cid", list(GEMM))
def test_gemm_simulation_passes(cid):
    c = GEMM[cid]
    d = R.gen_gemm(c)
    assert passes(R.expect_gemm(c, d), R.simulate_gemm(c, d), R.gemm_inits(c))


def test_gemm_reference_matches_autograd():
    """The float64 reference is the input gradient of torch's linear, and gelu_slope64 the derivative of its erf GELU."""
    c = GEMM["65x17x65-none-f32-f32"]
    d = R.gen_gemm(c)
    x = torch.zeros(c.M, c.K, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.linear(x, torch.from_numpy(d["w"]).double()).backward(torch.from_numpy(d["dy"]).double())
    assert np.abs(R.expect_gemm(c, d)["linear_dgrad.out"].ref - x.grad.numpy()).max() < 1e-12
    a = torch.linspace(-7.5, 7.5, 301, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.gelu(a).sum().backward()
    q, eq = R.gelu_slope64(a.detach().numpy())
    assert np.abs(q - a.grad.numpy()).max() < 1e-14 and eq.max() < 12 * R.U and (eq > 0).all()


# ------------------------------------------------------------------------------------------------ mutants
SPLIT_MUTANTS = [("B3L5D8-cls-f32", "slice_off_by_one"), ("B67L17D192-patch-bf16", "slice_off_by_one"), ("B300L3D1024-cls-f32", "slice_off_by_one"),
                 ("B3L5D8-patch-f32", "drop_u_tail"), ("B300L3D1024-cls-bf16", "drop_u_tail"), ("B60L50D768-patch-f32", "drop_u_tail"),
                 ("B5L17D192-cls-bf16", "copy_cls_row"), ("B1L1D4-cls-f32", "copy_cls_row"), ("B9L145D384-cls-f32", "dcls_row1"), ("B3L5D8-cls-bf16", "dcls_row1")]


@pytest.mark.parametrize("cid,mutate", SPLIT_MUTANTS)
def test_split_mutants_fail(cid, mutate):
    c = SPLIT[cid]
    for exact in (False, True):
        d = R.gen_split(c, exact)
        got = R.simulate_split(c, d, mutate)
        assert not passes(R.expect_split(c, d, exact), got, R.split_inits(c), R.split_extra(c, got)), (cid, mutate, exact)


def test_split_checks_catch_single_elements():
    c = SPLIT["B5L17D192-patch-f32"]
    d = R.gen_split(c, True)
    e, init = R.expect_split(c, d, True), R.split_inits(c)
    good = R.simulate_split(c, d)
    assert passes(e, good, init, R.split_extra(c, good))
    for name, at, val in (("full_grad_split.dpos", (0, 3), -0.0), ("full_grad_split.dcls", (5,), -0.0), ("full_grad_split.dpos", (c.pos_rows, 0), 0.0),
                          ("full_grad_split.dtok", (c.B * c.L, 0), 1.0), ("full_grad_split.partial", (R.slices(c.B, c.L, c.D) * c.L * c.D,), 0.0)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[name][at] = val
        assert not passes(e, bad, init, R.split_extra(c, bad)), (name, at)
    bad = {k: v.copy() for k, v in good.items()}
    bad["full_grad_split.dpos"][4, 7] += 1.0                                  # one image's integer too many
    assert not passes(e, bad, init, R.split_extra(c, bad))
    c = SPLIT["B5L17D192-cls-bf16"]
    d = R.gen_split(c)
    good = R.simulate_split(c, d)
    bad = {k: v.copy() for k, v in good.items()}
    bad["full_grad_split.dtok"][40, 3] ^= 1                                   # one bf16 ulp
    assert not passes(R.expect_split(c, d), bad, R.split_inits(c), R.split_extra(c, bad))
    bad = {k: v.copy() for k, v in good.items()}
    bad["full_grad_split.dcls"][3] = np.nextafter(bad["full_grad_split.dcls"][3], np.float32(9))   # inside the bound, but no copy of dpos[0]
    assert not passes(R.expect_split(c, d), bad, R.split_inits(c), R.split_extra(c, bad))


@pytest.mark.parametrize("cid,mutate", [("D8-L5-f32", "mod_L_plus_1"), ("D260-L5-bf16", "mod_L_plus_1"), ("D8-L1-f32", "mod_L_plus_1"), ("D8-trip-f32", "no_last_trip"),
                                        ("D260-trip-bf16", "no_last_trip"), ("D1024-L5-f32", "one_lane_pass"), ("D1024-L5-bf16", "one_lane_pass")])
def test_zero_mutants_fail(cid, mutate):
    c = ZERO[cid]
    d = R.gen_zero(c)
    assert not passes(R.expect_zero(c, d), R.simulate_zero(c, d, mutate), R.zero_inits(c, d))


def test_zero_checks_catch_a_negative_zero_and_a_guard_row():
    c = ZERO["D256-L5-bf16"]
    d = R.gen_zero(c)
    e, init, good = R.expect_zero(c, d), R.zero_inits(c, d), R.simulate_zero(c, d)
    for name, at, val in (("zero_token_rows.dres", (1, 0), -0.0), ("zero_token_rows.dres_c", (2, 255), 0x8000), ("zero_token_rows.dres", (c.rows, 0), 0.0),
                          ("zero_token_rows.dres_c", (5, 9), 0)):
        bad = {k: v.copy() for k, v in good.items()}
        bad[name][at] = val
        assert not passes(e, bad, init), (name, at)


POOL_MUTANTS = [("D192-s10r1_4-f32-none", "divide_by_seq"), ("D260-s10r1_10-bf16-none", "divide_by_seq"), ("D8-s10r0_1-f32-none", "divide_by_seq"),
                ("D260-s10r1_4-const", "divide_by_seq"), ("D260-s10r0_10-f32-none", "skip_last_column"), ("D256-s10r1_10-bf16-l2", "skip_last_column"),
                ("D1024-s10r1_6-f32-l2", "skip_last_column"), ("D4-s1r0_1-f32-none", "skip_last_column"), ("D768-s10r1_9-bf16-none", "waves_of_three"),
                ("D8-s10r2_6-f32-l2", "waves_of_three"), ("D1024-s10r1_10-const", "waves_of_three")]


@pytest.mark.parametrize("cid,mutate", POOL_MUTANTS)
def test_pool_mutants_fail(cid, mutate):
    c = POOL[cid]
    d = R.gen_pool(c)
    assert not passes(R.expect_pool(c, d), R.simulate_pool(c, d, mutate), R.pool_inits(c))


def test_pool_l2_hides_a_wrong_divisor_and_the_table_knows():
    """Under L2 the divisor cancels: divide_by_seq is a mutant only the un-normalised cases can see, which is why every range has one."""
    c = POOL["D192-s10r1_4-f32-l2"]
    d = R.gen_pool(c)
    assert passes(R.expect_pool(c, d), R.simulate_pool(c, d, "divide_by_seq"), R.pool_inits(c))
    assert all(any(k.kind == "random" and not k.l2 and (k.D, k.seq, k.lo, k.hi) == (c.D, c.seq, c.lo, c.hi) for k in POOL.values()) for c in POOL.values())


@pytest.mark.parametrize("cid", list(ELEM))
def test_cast_and_add_into_mutants_fail(cid):
    c = ELEM[cid]
    d = R.gen_cast(c, "f32")
    assert not passes(R.expect_cast(c, d, "f32", "bf16"), R.simulate_cast(c, d, "f32", "bf16", "truncate"), R.cast_inits(c, "bf16"))
    d = R.gen_add_into(c, "bf16")
    assert not passes(R.expect_add_into(c, d), R.simulate_add_into(c, d, "truncate"), R.add_into_inits(c, d))
    if c.n > R.ELEM_TRIP:
        for src, dst in R.DT_PAIRS:
            d = R.gen_cast(c, src)
            assert not passes(R.expect_cast(c, d, src, dst), R.simulate_cast(c, d, src, dst, "no_last_trip"), R.cast_inits(c, dst))
        for dt in ("f32", "bf16"):
            d = R.gen_add_into(c, dt)
            assert not passes(R.expect_add_into(c, d), R.simulate_add_into(c, d, "no_last_trip"), R.add_into_inits(c, d))


@pytest.mark.parametrize("cid,mutate", [("r7L3D4", "mod_L_plus_1"), ("r10L10D192", "mod_L_plus_1"), ("r4100L145D1024", "mod_L_plus_1"), ("r4100L145D1024", "no_last_trip")])
def test_pos_mutants_fail(cid, mutate):
    c = POS[cid]
    d = R.gen_pos(c)
    if cid == "r10L10D192":     # rows = L: r % (L + 1) = r, the mutant is invisible here and the longer cases carry it
        assert passes(R.expect_pos(c, d), R.simulate_pos(c, d, mutate), R.pos_inits(c))
        return
    assert not passes(R.expect_pos(c, d), R.simulate_pos(c, d, mutate), R.pos_inits(c))


GEMM_MUTANTS = [(f"{shape}-{mode}-{types}", "cut_at_16") for shape in ("31x20x24", "65x17x65", "1x1x1") for mode in ("none", "dgelu", "mul")
                for types in ("f32-f32", "bf16-bf16", "bf16-f32")]
GEMM_MUTANTS += [(f"{shape}-none-{types}", "last_column") for shape in ("65x17x65", "130x384x150", "1x1x1") for types in ("f32-f32", "bf16-bf16")]
GEMM_MUTANTS += [(f"64x16x64-{mode}-{types}", "aux_transposed") for mode in ("dgelu", "mul") for types in ("f32-f32", "bf16-bf16", "bf16-f32")]


@pytest.mark.parametrize("cid,mutate", GEMM_MUTANTS)
def test_gemm_mutants_fail(cid, mutate):
    c = GEMM[cid]
    d = R.gen_gemm(c)
    assert not passes(R.expect_gemm(c, d), R.simulate_gemm(c, d, mutate), R.gemm_inits(c))


def test_gemm_bound_is_a_few_ulps_not_a_tolerance():
    """One term of the 1536-long reduction dropped, and a single-precision slip of 64 ulps, both fail; the bound stays below
    N u sum|dy w| (1 + small) and above the error of the plain evaluation."""
    c = GEMM["70x1536x384-none-f32-f32"]
    d = R.gen_gemm(c)
    e, init, good = R.expect_gemm(c, d), R.gemm_inits(c), R.simulate_gemm(c, d)
    ratios, fails = R.judge(e, good, init)
    assert not fails and ratios["linear_dgrad.out"] < 0.25
    d2 = dict(d, dy=d["dy"].copy())
    d2["dy"][:, 777] = 0
    assert not passes(e, R.simulate_gemm(c, d2), init)
    bad = {k: v.copy() for k, v in good.items()}
    big = np.unravel_index(np.argmax(np.abs(e["linear_dgrad.out"].ref) / e["linear_dgrad.out"].bound), e["linear_dgrad.out"].ref.shape)
    bad["linear_dgrad.out"][big] *= np.float32(1 + 2.0 ** -8)
    assert not passes(e, bad, init)
