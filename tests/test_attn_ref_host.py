"""tests/attn_ref.py without a GPU: the reference against torch, the restated dispatch against the constants the kernels imply, the
honest-kernel emulation inside every bound on every input family, the exact claims of the routing and counting inputs, and every
mutant rejected by the check named for it."""
import dataclasses
import math

import pytest
import torch
import torch.nn.functional as F

from tests import attn_ref as R

BF = torch.bfloat16
EMU_SHAPES = [(1, 32), (17, 32), (33, 64), (36, 64), (81, 24), (145, 32), (145, 64), (197, 24), (257, 64)]   # (T, hd): table shapes
WORST = {}   # (family, output) -> worst ratio of the emulation


def _case(T, hd, B=2, H=3):
    return R.Case("bf16", B, T, H, hd)


def _emulate(c, qkv, do, r, mut=None, forms=None):
    rt = c.route
    online, dpm = forms if forms is not None else (rt.fwd.nch_t == 0, rt.bwd.dform == "DPM")
    f = dataclasses.replace(rt.fwd, nch_t=0 if online else rt.fwd.chunks)
    b = dataclasses.replace(rt.bwd, dform="DPM" if dpm else "dO.O")
    oin, lin = r.backward_inputs(BF)
    out, lse, dqkv = R.emulate_mfma(qkv, do, c.H, c.hd, online=online, dpm=dpm, out_in=oin, lse_in=lin, mut=mut)
    return f, b, out, lse, dqkv


def _note(family, reps):
    for k, rep in reps.items():
        WORST[(family, k)] = max(WORST.get((family, k), 0.0), rep.worst_ratio)


# ------------------------------------------------------------------------------------------------ reference
@pytest.mark.parametrize("T,hd", [(5, 16), (36, 24), (70, 64)])
def test_reference_matches_torch_autograd_and_sdpa(T, hd):
    c = _case(T, hd)
    qkv, do = (x.double() for x in R.gen_random(c, 1, torch.float32))
    r = R.reference(qkv, do, c.H, hd)
    x = qkv.clone().requires_grad_(True)
    q, k, v = R.split_heads(x, c.H, hd, 3)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    o = R.merge_heads(s.softmax(-1) @ v)
    o.backward(do)
    assert torch.allclose(R.merge_heads(r.O), o, rtol=0, atol=1e-13)
    assert torch.allclose(r.lse, torch.logsumexp(s, -1), rtol=0, atol=1e-13)
    assert torch.allclose(R.merge_heads(r.dQ, r.dK, r.dV), x.grad, rtol=0, atol=1e-12)
    y = qkv.clone().requires_grad_(True)
    o2 = R.merge_heads(F.scaled_dot_product_attention(*R.split_heads(y, c.H, hd, 3)))
    o2.backward(do)
    assert torch.allclose(R.merge_heads(r.O), o2, rtol=0, atol=1e-12)
    assert torch.allclose(R.merge_heads(r.dQ, r.dK, r.dV), y.grad, rtol=0, atol=1e-11)


# ------------------------------------------------------------------------------------------------ dispatch
def test_lds_sizes_and_thresholds():
    """The sizes the launchers ask for, recomputed by hand from the row stride 2 HD + 32, 1 KiB image granules and 2 Tp floats."""
    K = 1024
    # hd = 64, rows of 160 bytes: Tp = 224 -> 35 KiB images, four of them and 1792 bytes fit 160 KiB; Tp = 256 -> 40 KiB, 162 KiB do not
    assert R.attn_image(224, 224, 160, False) == (224, 35 * K) and R.attn_bwd_lds(0, 35 * K, 224) == 140 * K + 1792
    assert R.attn_image(256, 256, 160, False) == (256, 40 * K) and R.attn_bwd_lds(0, 40 * K, 256) == 160 * K + 2048 > R.LDS_BYTES
    assert R.attn_fwd_lds(False, R.attn_image(320, 320, 160, False)[1]) == 150 * K and R.attn_fwd_lds(False, R.attn_image(352, 352, 160, False)[1]) == 165 * K
    assert R.attn_fwd_lds(True, 80 * K) == 160 * K and R.attn_image(512, 512, 160, False)[1] == 80 * K       # FQ holds up to Tp = 512
    assert R.attn_bwd_lds(1, 75 * K, 480) == 150 * K + 3840 and R.attn_bwd_lds(2, 80 * K, 512) > R.LDS_BYTES    # two launches up to Tp = 480
    # hd = 32 (and the padded 24), rows of 96 bytes
    assert R.attn_bwd_lds(0, R.attn_image(416, 416, 96, False)[1], 416) == 4 * 39 * K + 3328 <= R.LDS_BYTES < R.attn_bwd_lds(0, R.attn_image(448, 448, 96, False)[1], 448)
    assert R.attn_fwd_lds(False, R.attn_image(544, 544, 96, False)[1]) == 153 * K <= R.LDS_BYTES < R.attn_fwd_lds(False, R.attn_image(576, 576, 96, False)[1])
    # trimmed images hold round_up(T, 16) rows
    assert R.attn_image(33, 64, 96, True) == (48, 5 * K) and R.attn_image(17, 32, 160, True) == (32, 5 * K) and R.attn_image(81, 96, 96, True) == (96, 9 * K)
    firsts = {hd: {} for hd in (24, 32, 64)}
    for hd in firsts:
        for T in range(1, 1025):
            rt = R.route("bf16", T, 2, hd)
            firsts[hd].setdefault(("fwd", rt.fwd.mfma, rt.fwd.fq), T)
            firsts[hd].setdefault(("bwd", rt.bwd.mfma, rt.bwd.ph), T)
    assert firsts[64][("bwd", True, 12)] == 225 and firsts[64][("fwd", True, True)] == 321
    assert firsts[64][("bwd", False, 0)] == 481 and firsts[64][("fwd", False, False)] == 513
    assert firsts[32][("bwd", True, 12)] == 417 and firsts[32][("fwd", True, True)] == 545
    assert firsts[32][("bwd", False, 0)] == 801 and firsts[32][("fwd", False, False)] == 833
    assert firsts[24][("bwd", False, 0)] == 417 and firsts[24][("fwd", False, False)] == 545 and ("fwd", True, True) not in firsts[24]


def test_threads_and_fallback_geometry():
    assert R.attn_threads(145, 512) == 320 and R.attn_threads(36, 512) == 192 and R.attn_threads(257, 512) == 384 and R.attn_threads(1024, 1024) == 1024
    assert R.generic_kb(600, 64, False) == 320 and R.generic_kb(600, 64, True) == 310 and R.generic_block(36) == 64 and R.generic_block(600) == 256


def test_routes_that_the_existing_parametrisation_claims():
    """The comments beside test_attention_fwd_bwd's shapes in tests/test_gpu_kernels.py."""
    for T, hd in ((257, 64), (304, 64), (480, 32)):           # backward as two launches
        assert R.route("bf16", T, 2, hd).bwd.ph == 12 and not R.route("bf16", T, 2, hd).fwd.fq
    for T, hd in ((500, 64), (700, 32)):                      # forward with Q from global memory
        assert R.route("bf16", T, 2, hd).fwd.fq
    rt = R.route("bf16", 600, 1, 64)                          # beyond that the block-streamed fallback
    assert not rt.fwd.mfma and not rt.bwd.mfma and rt.fwd.blocks == 2 and rt.bwd.blocks == 2
    assert R.route("bf16", 20, 2, 64).label[0] == "mfma<64,1,->" and R.route("bf16", 20, 2, 64).bwd.label[0] == "mfma<64,1,PH=0>"
    for T, hd in ((80, 32), (81, 24)):
        rt = R.route("bf16", T, 3, hd)
        assert rt.fwd.label[0] == "mfma<32,3,->" and rt.bwd.label[0] == "mfma<32,3,PH=0>" and rt.fwd.padded == (hd == 24)
    assert R.route("bf16", 145, 6, 32).fwd.nch_t == 5 and R.route("bf16", 145, 6, 32).bwd.nch_t == 0
    assert not R.route("f32", 36, 6, 64).fwd.mfma and not R.route("bf16", 36, 6, 64, aligned=False).bwd.mfma


def test_coverage_is_complete_and_the_table_is_small():
    assert R.coverage_gaps() == []
    assert R.coverage_gaps(tuple(c for c in R.cases() if c.T != 225))   # the checker notices a missing label
    firsts = {(T, dt, hd) for T, dt, hd in R.universe().values()}
    for c in R.cases():
        assert c.B * c.H <= 16
        assert c.T <= 900 or (c.T, c.dtype, c.hd) in firsts, c.id
    # the plain D loop in one launch: no shape reaches it (UNREACHABLE gives the arithmetic)
    assert not any(lbl[-1] == "loop" and "PH=0" in lbl[4] for lbl in R.universe())
    assert any(lbl[-1] == "loop" for lbl in R.universe()) and any(lbl[-1] == "prefetch" for lbl in R.universe())


# ------------------------------------------------------------------------------------------------ the emulation inside the bounds
@pytest.mark.parametrize("T,hd", EMU_SHAPES)
def test_emulation_stays_inside_every_bound(T, hd):
    c = _case(T, hd)
    for sigma in (1, 3):
        qkv, do = R.gen_random(c, sigma, BF)
        r = R.reference(qkv, do, c.H, hd)
        for forms in (None, (True, False), (False, True)):   # the case's own forms, then online + dO.O and two-pass + DPM
            f, b, out, lse, dqkv = _emulate(c, qkv, do, r, forms=forms)
            reps = {**R.check_fwd(r, f, out, lse), **R.check_bwd(r, b, dqkv)}
            _note(f"sigma={sigma}", reps)
            for rep in reps.values():
                assert rep.ok, str(rep)


@pytest.mark.parametrize("T,hd", EMU_SHAPES)
def test_routing_is_exact_on_the_emulation(T, hd):
    c = _case(T, hd)
    qkv, do, sigma, want_out, want_dv, lse_exact = R.gen_routing(c, BF)
    r = R.reference(qkv, do, c.H, hd)
    assert float((r.lse - lse_exact).abs().max()) < 1e-12 * max(1.0, lse_exact)
    for forms in (None, (True, False), (False, True)):
        f, b, out, lse, dqkv = _emulate(c, qkv, do, r, forms=forms)
        assert R.exact_mismatches(out, want_out) == 0
        assert R.exact_mismatches(R.split_heads(dqkv, c.H, hd, 3)[2].contiguous(), want_dv) == 0
        reps = {**R.check_fwd(r, f, out, lse), **R.check_bwd(r, b, dqkv)}
        _note("routing", reps)
        for rep in reps.values():
            assert rep.ok, str(rep)


@pytest.mark.parametrize("T,hd", EMU_SHAPES)
def test_counting_on_the_emulation(T, hd):
    c = _case(T, hd)
    qkv, count = R.gen_counting(c, BF)
    do = torch.zeros(c.B, T, c.H * hd, dtype=BF)
    r = R.reference(qkv, do, c.H, hd)
    for forms in (None, (True, False)):
        f, b, out, lse, _ = _emulate(c, qkv, do, r, forms=forms)
        reps = R.check_counting(r, f, out, lse, count)
        _note("counting", reps)
        for rep in reps.values():
            assert rep.ok, str(rep)


# ------------------------------------------------------------------------------------------------ mutants
def test_mutant_key_past_T_unmasked():
    c = _case(33, 32)
    qkv, count = R.gen_counting(c, BF)
    do = torch.zeros(c.B, 33, c.H * 32, dtype=BF)
    r = R.reference(qkv, do, c.H, 32)
    f, b, out, lse, _ = _emulate(c, qkv, do, r, mut={"unmask": True})
    reps = R.check_counting(r, f, out, lse, count)
    assert reps["out"].bad > 0 and reps["lse"].bad == c.B * c.H * 33
    qkv, do, sigma, want_out, want_dv, _ = R.gen_routing(c, BF)
    r = R.reference(qkv, do, c.H, 32)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r, mut={"unmask": True})
    bad = R.check_fwd(r, f, out, lse)["lse"]       # key 32 counted 32 times: its query's lse moves by log 32, its out does not
    assert bad.bad == c.B * c.H and bad.worst[2] == int(torch.argsort(sigma[bad.worst[0], bad.worst[1]])[32])


def test_mutant_dk_without_scale_in_one_head():
    c = _case(36, 64)
    qkv, do = R.gen_random(c, 1, BF)
    r = R.reference(qkv, do, c.H, 64)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r)
    dq, dk, dv = (x.clone() for x in R.split_heads(dqkv, c.H, 64, 3))
    dk[1, 2] = (dk[1, 2].float() * 8).to(BF)
    reps = R.check_bwd(r, b, R.merge_heads(dq, dk, dv))
    assert reps["dK"].bad > 0.9 * 36 * 64 and reps["dK"].first_bad[:2] == (1, 2) and reps["dQ"].ok and reps["dV"].ok


@pytest.mark.parametrize("dpm", [False, True])
def test_mutant_d_from_the_neighbouring_query(dpm):
    c = _case(36, 64)
    qkv, do = R.gen_random(c, 3, BF)
    r = R.reference(qkv, do, c.H, 64)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r, mut={"d_shift": 1}, forms=(False, dpm))
    reps = R.check_bwd(r, b, dqkv)
    assert reps["dQ"].bad > 0 and reps["dQ"].first_bad[2] // 16 == 1 and reps["dK"].bad > 0 and reps["dV"].ok


def test_mutant_lse_without_its_maximum():
    c = _case(145, 32)
    qkv, do = R.gen_random(c, 1, BF)
    r = R.reference(qkv, do, c.H, 32)
    f, b, out, lse, _ = _emulate(c, qkv, do, r)
    lse = lse.clone()
    lse[1, 0, 77] -= r.M[1, 0, 77].float()
    rep = R.check_fwd(r, f, out, lse)["lse"]
    assert rep.bad == 1 and rep.first_bad == (1, 0, 77, None)
    lse[1, 0, 77] = r.lse[1, 0, 77].float() + 0.01       # and an lse that is off by 0.01
    assert R.check_fwd(r, f, out, lse)["lse"].bad == 1


def test_mutants_of_the_routing_check():
    c = _case(81, 24)
    qkv, do, sigma, want_out, want_dv, _ = R.gen_routing(c, BF)
    r = R.reference(qkv, do, c.H, 24)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r)
    o = R.split_heads(out, c.H, 24).clone()
    o[1, [0, 1]] = o[1, [1, 0]]                                               # heads h and h + 1 swapped in one image
    assert R.exact_mismatches(R.merge_heads(o), want_out) > 70 * 2 * 24
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r, mut={"pv_swap": 1})        # keys 36-39 and 48-51 swapped in P V
    assert R.exact_mismatches(out, want_out) == c.B * c.H * 8 * 24


def test_mutant_query_tile_not_written():
    c = _case(36, 64)
    qkv, do = R.gen_random(c, 1, BF)
    r = R.reference(qkv, do, c.H, 64)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r)
    buf, view = R.guarded(out.shape, BF)
    view.copy_(out)
    view[1, 16:32, 64:128] = R.fill_like((16, 64), BF)
    rep = R.check_fwd(r, f, view, lse)["out"]
    assert rep.fill == 16 * 64 and rep.nan == 0 and not rep.ok and rep.first_bad == (1, 1, 16, 0) and R.guards_touched(buf, view) == 0


def test_mutant_hd24_head_writes_eight_columns_into_its_neighbour():
    c = _case(17, 24)
    qkv, do = R.gen_random(c, 1, BF)
    r = R.reference(qkv, do, c.H, 24)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r)
    buf, view = R.guarded(out.shape, BF)
    view.copy_(out)
    flat = buf[R.GUARD:]
    for row in range(c.B * 17):          # every head stores its zero-padded columns 24..31 as well, in head order
        for h in range(c.H):
            flat[row * c.H * 24 + h * 24 + 24:row * c.H * 24 + h * 24 + 32] = 0
    assert R.guards_touched(buf, view) == 8
    rep = R.check_fwd(r, f, view, lse)["out"]
    assert rep.bad > 0 and rep.first_bad[3] < 8


def test_mutant_one_element_moved_by_two_bf16_ulps():
    c = _case(145, 32)
    qkv, do = R.gen_random(c, 3, BF)
    r = R.reference(qkv, do, c.H, 32)
    f, b, out, lse, dqkv = _emulate(c, qkv, do, r)
    e = R.bounds_fwd(r, f)[0]
    o = R.split_heads(out, c.H, 32).clone()
    pick = ((r.O.abs() >= 1) & (r.O.abs() < 2)).double() / e      # an O(1) element whose bound is the tightest
    i = tuple(int(x) for x in (pick == pick.max()).nonzero()[0])
    assert float(e[i]) < 2.0 ** -7
    for step in (2, -2):
        m = o.clone()
        m[i] = R._key_to_double(R._bf16_key(o[i]) + step).to(BF)
        rep = R.check("out", m, r.O, e)
        assert rep.bad == 1 and rep.first_bad == i, str(rep)


def test_zz_emulation_ratios():
    print("\nworst error / bound of the emulation per input family and output:")
    for (fam, k), v in sorted(WORST.items()):
        print(f"  {fam:9s} {k:4s} {v:.3f}")
    assert all(v < 1 for v in WORST.values())
