"""The optimizer reference (tests/optim_ref.py) checked on the host: the fp64 formulas against torch, the bounds against an
fp32 emulation of adamw_kernel in its own operation order, and the proof that the bounds tell wrong kernels apart: every
mutant of the emulation leaves a bound on the data the GPU test uses."""
import math

import numpy as np
import pytest
import torch

from tests import optim_ref as R

N = 1 << 18
F = np.float32


def _fma(a, b, c):
    """fl(a b + c) in one rounding: the product of two fp32 numbers is exact in double."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(F)


def emulate(c, fma=False, mutant=None):
    """adamw_kernel<true, false> in fp32, operation by operation (launch_adamw's host arithmetic included).  fma = the
    contractions -ffp-contract=fast allows.  Returns (p', m', v', bf16 bits of the straight copy)."""
    lr, b1, b2, eps, wd = F(c["lr"]), F(c["b1"]), F(c["b2"]), F(c["eps"]), F(c["wd"])
    bc1, bc2 = F(1.0 - float(b1) ** c["step"]), F(1.0 - float(b2) ** c["step"])
    inv_bc1, inv_sqrt_bc2 = F(1) / bc1, F(1) / np.sqrt(bc2)
    coef = F(1) if mutant == "coef_ignored" else F(c["coef"])
    decay, step = F(1) - lr * wd, lr * inv_bc1
    p, g, m, v = c["p"], c["g"], c["m"], c["v"]
    gg = g * coef
    if mutant == "l2_decay":
        gg = gg + wd * p
    pp = p if mutant == "decay_after" else p * decay
    bm = b2 if mutant == "b2_for_m" else b1
    if fma:
        mm = _fma(m, bm, gg * (F(1) - bm))
        vv = _fma(v, b2, gg * gg * (F(1) - b2))
    else:
        mm = m * bm + gg * (F(1) - bm)
        vv = v * b2 + gg * gg * (F(1) - b2)
    if mutant == "eps_before_bc":
        denom = (np.sqrt(vv) + eps) * inv_sqrt_bc2
    elif mutant == "v_uncorrected":
        denom = np.sqrt(vv) + eps
    elif fma:
        denom = _fma(np.sqrt(vv), inv_sqrt_bc2, np.full_like(vv, eps))
    else:
        denom = np.sqrt(vv) * inv_sqrt_bc2 + eps
    q = mm / denom
    pp = _fma(q, -step, pp) if fma else pp - step * q
    if mutant == "decay_after":
        pp = pp * decay
    assert pp.dtype == F and mm.dtype == F and vv.dtype == F
    wbf = R.bf16_truncate(pp) if mutant == "bf16_truncated" else R.bf16_rne(p if mutant == "bf16_stale" else pp)
    return pp, mm, vv, wbf


def verdict(c, out):
    """Worst ratio over p', m', v'; infinite if the bf16 copy is not bf16_rne of the fp32 p' that was written."""
    pp, mm, vv, wbf = out
    worst = max(R.adamw_ratios(pp, mm, vv, c).values())
    return worst if np.array_equal(wbf, R.bf16_rne(pp)) else math.inf


@pytest.fixture(scope="module")
def cases():
    return {h: R.gen_case(N, h, seed=11) for h in R.HYPER}


def test_adamw_equals_torch_adamw_over_three_steps():
    g = torch.Generator().manual_seed(5)
    lr, wd = R.f32(1e-3), R.f32(0.05)
    betas, eps = (R.f32(R.B1), R.f32(R.B2)), R.f32(R.EPS)
    w = torch.randn(4096, dtype=torch.float64, generator=g).requires_grad_()
    opt = torch.optim.AdamW([w], lr=lr, betas=betas, eps=eps, weight_decay=wd)
    p, m, v = w.detach().numpy().copy(), np.zeros(4096), np.zeros(4096)
    for step in (1, 2, 3):
        grad = torch.randn(4096, dtype=torch.float64, generator=g) * 10.0 ** torch.randint(-6, 2, (4096,), generator=g).double()
        w.grad = grad.clone()
        opt.step()
        p, m, v = R.adamw(p, grad.numpy(), m, v, 1.0, lr, betas[0], betas[1], eps, wd, step)
        st = opt.state[w]
        for ours, theirs in ((p, w.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
            np.testing.assert_allclose(ours, theirs.numpy(), rtol=1e-12, atol=1e-300)


def test_coef_scales_the_gradient():
    c = R.gen_case(1024, "step2", seed=3)
    a = R.adamw(c["p"], c["g"], c["m"], c["v"], 0.37, **R.hyper_args(c))
    b = R.adamw(c["p"], c["g"].astype(np.float64) * 0.37, c["m"], c["v"], 1.0, **R.hyper_args(c))
    for x, y in zip(a, b):
        np.testing.assert_allclose(x, y, rtol=1e-15, atol=0)


@pytest.mark.parametrize("max_norm", [1.0, 0.01, 1e6, math.inf])
def test_clip_equals_clip_grad_norm(max_norm):
    max_norm = R.f32(max_norm)    # what the C ABI passes
    g = torch.Generator().manual_seed(9)
    ws =[torch.zeros(n, dtype=torch.float64).requires_grad_() for n in (100, 37, 1000)]
    for w in ws:
        w.grad = torch.randn(w.shape, dtype=torch.float64, generator=g)
    flat = torch.cat([w.grad for w in ws]).numpy().copy()
    total = torch.nn.utils.clip_grad_norm_(ws, max_norm)
    norm, coef = R.clip(R.sumsq(flat), max_norm)
    assert abs(norm - float(total)) <= 1e-12 * norm
    np.testing.assert_allclose(flat * coef, torch.cat([w.grad for w in ws]).numpy(), rtol=1e-12, atol=0)
    assert R.clip(0.0, 1.0) == (0.0, 1.0) and R.clip(4.0, math.inf) == (2.0, 1.0)


def test_ema_and_its_bound():
    r = np.random.default_rng(2)
    t, p = r.standard_normal(4096).astype(F), r.standard_normal(4096).astype(F)
    assert np.array_equal(R.ema(t, p, 1.0), t.astype(np.float64)) and np.array_equal(R.ema(t, p, 0.0), p.astype(np.float64))
    for mom in (0.996, 0.3):
        out = t * F(mom) + p * (F(1) - F(mom))
        ref, bound = R.ema(t, p, mom), R.ema_bound(t, p, mom)
        assert R.worst_ratio(out, ref, bound) <= 1.0
        assert R.worst_ratio(t * F(mom) + p * F(mom), ref, bound) > 1.0    # a wrong weight is seen
    assert np.all(R.ema_bound(t, p, 1.0) >= 0)


def test_bf16_rne_is_torch_bfloat16():
    r = np.random.default_rng(4)
    bits = r.integers(0, 1 << 32, 1 << 20, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3F817FFF, 0x3F818001, 0x00000000, 0x80000000, 0x7F7FFFFF,
                        0xFF7FFFFF, 0x00800000, 0x80800000, 0x7F800000, 0xFF800000, 0x00000001, 0x00008000, 0x7F7F8000, 0x7F7F7FFF],
                       dtype=np.uint32)
    bits = np.concatenate([special, bits])
    x = bits.view(F)
    finite = ~np.isnan(x)
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = R.bf16_rne(x)
    assert np.array_equal(got[finite], want[finite])
    assert np.all((got[~finite] & 0x7FC0) == 0x7FC0)   # a NaN stays a (quiet) NaN
    # ties: even upper half stays, odd upper half goes up; the largest finite fp32 overflows to infinity
    assert list(got[:3]) == [0x3F80, 0x3F82, 0x3F81] and got[8] == 0x7F80
    assert np.array_equal(R.bf16_truncate(x[:6]), np.array([0x3F80, 0x3F81, 0x3F80, 0x3F80, 0x3F81, 0x3F81], dtype=np.uint16))


def emulate_sumsq(g):
    """sumsq_kernel -> block_sum_256 -> sumsq_finalize_kernel in fp32, addition by addition."""
    n4 = g.size // 4
    grid = max(1, min(-(-n4 // 256), R.RED_BLOCKS))
    threads = grid * 256
    passes = max(1, -(-n4 // threads))
    v = np.zeros((passes * threads, 4), F)
    v[:n4] = g.reshape(-1, 4)
    sq = v * v
    acc = np.zeros(threads, F)
    for term in (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]).reshape(passes, threads):
        acc = acc + term

    def block_sum(x):   # (blocks, 256): the xor butterfly of wave_sum in each of the four waves, then red[0] + .. + red[3]
        w = x.reshape(-1, 4, 64)
        for o in (32, 16, 8, 4, 2, 1):
            w = w + w[..., np.arange(64) ^ o]
        return ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]

    partial = np.zeros(-(-grid // 256) * 256, F)
    partial[:grid] = block_sum(acc.reshape(grid, 256))
    fin = np.zeros(256, F)
    for row in partial.reshape(-1, 256):
        fin = fin + row
    out = block_sum(fin.reshape(1, 256))[0]
    assert out.dtype == F
    return float(out)


@pytest.mark.parametrize("n", [4, 1020, 1024 * 300, R.SUMSQ_WRAP + 4, 2 * R.SUMSQ_WRAP + 1028])
def test_sumsq_emulation_stays_inside_the_counted_chain(n):
    g = R.gen_grad(n, seed=n)
    ref = R.sumsq(g)
    ratio = abs(emulate_sumsq(g) - ref) / (R.sumsq_rel_bound(n) * ref)
    print(f"n={n}: chain {R.sumsq_chain(n)}, error / bound {ratio:.3f}")
    assert ratio <= 1.0
    ones = np.ones(n, F)     # exact in fp32: the emulation counts every element once
    assert emulate_sumsq(ones) == n


def test_sumsq_chain_counts():
    assert R.sumsq_chain(0) == 0 + 1 + 22 and R.sumsq_chain(4) == 1 + 1 + 22
    assert R.sumsq_chain(R.SUMSQ_WRAP) == 1 + 4 + 22 and R.sumsq_chain(R.SUMSQ_WRAP + 4) == 2 + 4 + 22
    assert R.sumsq_chain(5_000_004) == 5 + 4 + 22
    assert R.sumsq_chain(1024 * 300) == 1 + 2 + 22
    assert R.norm_rel_bound(28) == R.SECOND * 15 * R.U and R.coef_rel_bound(28) == R.SECOND * 17 * R.U


def test_wcache_layout_on_a_hand_written_table():
    T, M, FROZEN = R.TRAINABLE, R.TRAINABLE | R.MATRIX, 2
    table = [
        ("unused", 900, 48, (1, 1, 48), 4),
        ("cls", 0, 48, (1, 1, 48), T),
        ("pos", 964, 100, (1, 25, 4), FROZEN),
        ("conv", 64, 48 * 12, (48, 3, 2, 2), M),       # 576 elements: a multiple of 64
        ("bias", 640, 48, (48,), T),
        ("qkv", 704, 12 * 4, (12, 4), M),              # 48 elements: padded to 64
        ("proj", 768, 4 * 20, (4, 20), M),             # 80 elements: padded to 128
    ]
    mats, trans = R.wcache_layout(table, 896)
    assert [m["name"] for m in mats] == ["conv", "qkv", "proj"]
    assert [(m["rows"], m["cols"]) for m in mats] == [(48, 12), (12, 4), (4, 20)]
    assert [m["t_off"] for m in mats] == [0, 576, 640] and trans == 768
    assert [m["t_abs"] for m in mats] == [896, 1472, 1536] and [m["offset"] for m in mats] == [64, 704, 768]
    arena = np.arange(1000, dtype=F)
    t = R.transposed_ref(arena, mats[2]).reshape(20, 4)
    assert np.array_equal(t, R.bf16_rne(arena[768:848].reshape(4, 20).T.copy()))
    assert t[1, 0] == R.bf16_rne(np.array([769], dtype=F))[0] and t[0, 1] == R.bf16_rne(np.array([788], dtype=F))[0]


def test_generated_data_is_what_the_issue_asks_for(cases):
    for h, c in cases.items():
        g, p = c["g"], c["p"]
        nz = np.abs(g[g != 0]).astype(np.float64)
        assert nz.min() >= 0.99e-12 and nz.max() <= 101.0 and (g == 0).sum() > N // 128 and (p == 0).sum() > N // 128
        tiny = float(np.finfo(F).tiny)
        assert ((1.0 - R.f32(R.B2)) * (nz * c["coef"]) ** 2).min() > tiny, "(1 - b2) g^2 must stay normal"
        assert not np.signbit(p[p == 0]).any()
        if c["step"] == 1:
            assert not c["m"].any() and not c["v"].any()
        else:
            stripe = np.arange(N) % 1024 == 300
            m2 = R.adamw_terms(p, g, c["m"], c["v"], c["coef"], **R.hyper_args(c))
            assert np.all(np.abs(m2["m"][stripe]) <= 1e-6 * m2["A"][stripe])           # cancellation
            assert np.abs(c["v"][c["v"] != 0]).min() > tiny and np.abs(c["m"][c["m"] != 0]).min() > tiny
        assert 0.3 < c["coef"] < 0.4


@pytest.mark.parametrize("fma", [False, True], ids=["separate", "fused"])
def test_faithful_emulation_passes_every_bound(cases, fma):
    for h, c in cases.items():
        pp, mm, vv, wbf = emulate(c, fma)
        r = R.adamw_ratios(pp, mm, vv, c)
        print(f"{h:7s} fma={int(fma)} p {r['p']:.3f} m {r['m']:.3f} v {r['v']:.3f}")
        assert max(r.values()) <= 1.0, (h, r)
        assert np.array_equal(wbf, R.bf16_rne(pp))


MUTANTS = ["eps_before_bc", "v_uncorrected", "decay_after", "l2_decay", "coef_ignored", "b2_for_m", "bf16_truncated", "bf16_stale"]


@pytest.mark.parametrize("mutant", MUTANTS)
def test_every_mutant_violates_a_bound(cases, mutant):
    caught = {h: verdict(c, emulate(c, False, mutant)) for h, c in cases.items()}
    print(mutant, {h: f"{v:.3g}" for h, v in caught.items()})
    assert any(v > 1.0 for v in caught.values()), caught
    assert all(verdict(c, emulate(c, False, None)) <= 1.0 for c in cases.values())
