"""tests/token_ref.py against independent code, on the CPU: the oracle's patchify / target / decoder-input assembly, torch float64
autograd for the adjoints, torch's own losses; the plain fp32 evaluation stays inside the reference's bounds; and the checkers
reject mutants of a correct result (a dropped or doubled row, a token id off by one, a wrong element order, one bf16 ulp, a
written guard row, a changed untouched row)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import token_ref as R

SMALL_ROWS = [c for c in R.row_cases() if c.dec_rows <= 4000]
SMALL_JEPA = [c for c in R.jepa_cases() if c.rows <= 4000]
SMALL_PIX = [c for c in R.loss_cases() if not c.lite]


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(R.from_dt(a))).double()


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_tables_reach_every_path():
    rows = R.row_cases()
    assert {c.D for c in rows} == set(R.DIMS) and [R.rpi(D) for D in R.DIMS] == [128, 7, 5, 1, 1]
    assert 256 - 7 * 36 == 4 and 256 - 192 == 64 and 256 - 256 == 0          # idle threads at 144, 768, 1024
    for D in R.DIMS:
        cs, stride = [c for c in rows if c.D == D], R.SPLIT_BLOCKS * R.rpi(D)
        for n in ("vis_rows", "dec_rows"):
            counts = {getattr(c, n) for c in cs}
            assert 1 in counts and 3 * R.rpi(D) in counts
            assert any(stride < r < 4 * stride and r % (4 * stride) for r in counts), "no U = 4 tail"
            assert any(r > 4 * stride for r in counts), "no second trip of the split kernels"
        assert 3 * R.rpi(D) + 1 in {c.dec_rows for c in cs}
        assert any(c.k == 1 for c in cs) and any(c.k == c.L and c.L > 1 for c in cs) and any(c.keep == "unsorted" for c in cs)
        assert {c.dtype for c in cs} == {"f32", "bf16"}
    assert any(c.D == 192 and c.dec_rows > 4 * R.ROW_BLOCKS * 5 and c.k < c.L for c in rows)
    assert any(c.D == 192 and c.vis_rows * 48 > R.ROW_BLOCKS * 256 for c in rows)
    assert (15 * 145 > 4 * 512) and any(c.D == 1024 and c.B == 15 for c in rows) and any(c.D == 192 and c.B == 71 for c in rows)
    jep = R.jepa_cases()
    assert {c.nblk for c in jep} == {1, 4} and {c.m for c in jep} == {1, 20}
    for D in R.DIMS:
        big = [c for c in jep if c.D == D and c.rows > R.ROW_BLOCKS * R.rpi(D)]
        assert big and all(min(c.B * c.k, c.B * c.nblk * c.m) > R.SPLIT_BLOCKS * R.rpi(D) for c in big)
    zer = R.zero_cases()
    assert {c.D for c in zer} == {192, 256, 264, 1024} and {c.m for c in zer if not c.use_inv} >= {0, 1, 50}
    assert any(c.B * c.T > R.ZERO_BLOCKS * 4 and c.D == 192 for c in zer) and any(c.B * c.T > R.ZERO_BLOCKS * 2 and c.D == 264 for c in zer)
    los, gat = R.loss_cases(), R.gather_cases()
    assert {(c.C, c.img, c.p) for c in los} == set(R.GEOS) | {(3, 1024, 16), (1, 260, 4)} == {(c.C, c.img, c.p) for c in gat}
    assert any(c.B * c.g > 1024 and R.band_f32_eligible(c.C, c.img, c.p, c.n) for c in los) and any(c.B * c.g > 4096 for c in gat)
    assert not R.band_f32_eligible(1, 28, 7, 12) and not R.band_f32_eligible(3, 42, 14, 5) and not R.band_f32_eligible(3, 1024, 16, 4096)
    assert not R.u8_supported(1, 260, 4, 6) and not R.u8_supported(1, 28, 7, 5) and not R.band_f32_eligible(1, 260, 4, 6)   # g > 64, p % 4
    assert 3 * 16 * 1024 + 4097 * 4 > 65536 and 3 * 16 * 1024 + 4096 * 8 > 65536       # the hipFuncSetAttribute branches
    assert {c.kind for c in los} >= {"random", "oneband", "emptyband", "oor"}
    ns = [c.n for c in R.sl1_cases()]
    assert 4 in ns and any(n // 4 <= 256 for n in ns) and 1024 * 1024 in ns and any(n > 1024 * 1024 for n in ns)
    for name, a in R.INDEX_TRIPS:
        n = a["B"] * a["n_per"] if name == "build_row_map" else a["seqs"] * a["m"] if name == "build_tail_row_map" else a["B"] * a["per_image"]
        assert n > R.IDX_BLOCKS * 256


def test_token_lists_do_what_their_kind_says():
    for c in R.loss_cases():
        tok, g = R.gen_pixels(c, False)["tok"], c.g
        band = np.clip(tok - 1, 0, g * g - 1) // g
        if c.kind == "oneband":
            assert (band == g - 1).all()
        if c.kind == "emptyband":
            assert not (band == 1).any()
        if c.kind == "oor":
            assert (tok == 0).any() and (tok == g * g + 1).any()
        else:
            assert tok.min() >= 1 and tok.max() <= g * g
    for c in R.gather_cases():
        tok = R.gen_pixels(c, True)["tok"]
        assert tok.min() >= 0 and tok.max() <= c.g * c.g
        if c.kind in ("random", "emptyband", "all") and not c.lite:
            assert (tok == 0).any()


# ------------------------------------------------------------------------------------------------ exactness premise
@pytest.mark.parametrize("c", [c for c in R.row_cases() if c.id in ("D8-trip-f32", "D192-tripall-f32", "D1024-tail-f32")], ids=lambda c: c.id)
def test_integer_sums_do_not_depend_on_the_order(c):
    d = R.gen_rows(c, exact=True)
    for x in (d["dx_vis"][d["keep"].reshape(-1) == 0], d["dx_dec"][(d["inv"] < 0).reshape(-1)]):
        ref = x.astype(np.float64).sum(0)
        fwd = np.add.accumulate(x, axis=0, dtype=np.float32)[-1] if len(x) else np.zeros(c.D, np.float32)
        bwd = np.add.accumulate(x[::-1], axis=0, dtype=np.float32)[-1] if len(x) else fwd
        pair = x.sum(0, dtype=np.float32)
        strided = sum((x[i::7].sum(0, dtype=np.float32) for i in range(7)), np.zeros(c.D, np.float32))
        for s in (fwd, bwd, pair, strided):
            assert s.dtype == np.float32 and np.array_equal(s.astype(np.float64), ref)
        assert np.abs(x).astype(np.float64).sum(0).max() < 2 ** 24


# ------------------------------------------------------------------------------------------------ against independent code
@pytest.mark.parametrize("geo", R.GEOS, ids=str)
def test_patch_orders_match_oracle_and_unfold(geo):
    C, img, p = geo
    c = R.PixCase("x", C, img, p, 2, 5, "random")
    d = R.gen_pixels(c, True)
    im = torch.from_numpy(d["f32"][:2])
    assert torch.equal(torch.from_numpy(R.patches_of(d["f32"][:2], p, "ppc")), O.patchify(im, p))
    assert torch.equal(torch.from_numpy(R.patches_of(d["f32"][:2], p, "cpp")), F.unfold(im, p, stride=p).transpose(1, 2))
    assert torch.equal(im, ((torch.from_numpy(d["u8"][:2]).float() / 255) - 0.5) / 0.5)          # norm_u8 == ToTensor + Normalize
    tok = torch.from_numpy(d["tok"]).long()
    rows = R.from_dt(R.expect_gather(c, d, "f32")["gather_patches.out"].want).reshape(2, 5, -1)
    for b in range(2):
        for j in range(5):
            t = int(tok[b, j])
            want = torch.zeros(C * p * p) if t == 0 else im[b, :, (t - 1) // c.g * p:(t - 1) // c.g * p + p, (t - 1) % c.g * p:(t - 1) % c.g * p + p].reshape(-1)
            assert torch.equal(torch.from_numpy(rows[b, j]), want)


@pytest.mark.parametrize("c", SMALL_PIX, ids=lambda c: c.id)
def test_mse_reference_matches_torch(c):
    d = R.gen_pixels(c, False)
    cfg = O.MAEConfig(image_size=c.img, patch_size=c.p, in_chans=c.C, embed_dim=8, depth=1, num_heads=1, decoder_embed_dim=8, decoder_depth=1,
                      decoder_num_heads=1)
    g2 = c.g * c.g
    idx = torch.from_numpy(d["tok"]).long().clamp(max=g2)                  # the oracle clamps from below only; g*g + 1 means g*g
    target = O.build_target(torch.from_numpy(d["f32"][:c.B]).double(), idx, cfg).reshape(-1, c.P)
    pred = torch.from_numpy(d["pred"]).double().requires_grad_()
    for gs in (1.0, 1.0 / 3.0):
        e = R.expect_mse(c, d, "gather", gs, "f32")
        loss = F.mse_loss(pred, target)
        (grad,) = torch.autograd.grad(loss * float(np.float32(gs)), pred)
        assert abs(e["mse.loss"].ref[0] - loss.item()) <= 1e-14 * loss.item()
        got = torch.from_numpy(e["mse.d_pred"].want).double()
        assert torch.all((got - grad).abs() <= 4 * R.U * grad.abs() + 1e-45)       # subtraction, two products, one division


@pytest.mark.parametrize("cid", ["c3i32p8-oor", "c1i28p7-random"])
def test_patchify_reference_matches_oracle(cid):
    c = next(x for x in R.loss_cases() if x.id == cid)
    d = R.gen_pixels(c, False)
    patches = O.patchify(torch.from_numpy(d["f32"][:c.B]), c.p)
    idx = (torch.from_numpy(d["tok"]).long() - 1).clamp(0, c.g * c.g - 1)
    want = torch.gather(patches, 1, idx.unsqueeze(-1).expand(-1, -1, c.P)).reshape(-1, c.P)
    got = R.expect_patchify(c, d)["patchify_gather.target"].want
    assert got.dtype == np.float32 and np.array_equal(R.bits(got), R.bits(want.numpy()))


@pytest.mark.parametrize("c", R.sl1_cases()[:3], ids=lambda c: c.id)
def test_smooth_l1_reference_matches_torch(c):
    d = R.gen_sl1(c)
    pred, target = torch.from_numpy(d["pred"]).double().requires_grad_(), torch.from_numpy(d["target"]).double()
    e = R.expect_sl1(c, d, 1.0 / 3.0, "f32")
    loss = F.smooth_l1_loss(pred, target, beta=1.0)
    (grad,) = torch.autograd.grad(loss * float(np.float32(1.0 / 3.0)), pred)
    assert abs(e["smooth_l1.loss"].ref[0] - loss.item()) <= 1e-14 * loss.item()
    got = torch.from_numpy(e["smooth_l1.d_pred"].want).double()
    assert torch.all((got - grad).abs() <= 3 * R.U * grad.abs() + 1e-45)
    n = len(R.SL1_SPECIALS) if c.n > 4 else 4
    assert np.array_equal(d["pred"][:n] - d["target"][:n], d["pred"][:n])      # the special differences are exact
    if c.n > 4:
        gs = np.float32(1.0 / 3.0) / np.float32(c.n)
        assert np.array_equal(e["smooth_l1.d_pred"].want[1:7], np.array([1, -1, R.ONE_M, -R.ONE_M, 1, -1], np.float32) * gs)


@pytest.mark.parametrize("c", SMALL_ROWS, ids=lambda c: c.id)
def test_row_references_match_torch_and_autograd(c):
    d = R.gen_rows(c)
    e = R.expect_rows(c, d)
    keep, mask = torch.from_numpy(d["keep"]).long(), torch.from_numpy(d["mask"]).long()
    B, L, k, D = c.B, c.L, c.k, c.D
    # encoder side: cat(cls) + pos_embed, then gather(idx_keep)  (oracle.forward_encoder); x holds the patch rows of the kept tokens
    x, cls, pos = t64(d["x"]).reshape(B, k, D).requires_grad_(), t64(d["cls"]).requires_grad_(), t64(d["pos"])
    full = torch.zeros(B, L, D, dtype=torch.float64).scatter(1, keep.unsqueeze(-1).expand(-1, -1, D), x)
    full = torch.cat([cls.expand(B, 1, D), full[:, 1:]], 1) + pos
    vis = torch.gather(full, 1, keep.unsqueeze(-1).expand(-1, -1, D))
    got = t64(e["assemble_visible.x"].want).reshape(B, k, D)
    assert torch.all((got - vis).abs() <= R.U * vis.abs())
    dx = t64(d["dx_vis"]).reshape(B, k, D)
    gx, gcls = torch.autograd.grad(vis, (x, cls), dx)
    assert torch.equal(t64(R.from_dt(R.to_dt(d["dx_vis"], "f32"))).reshape(B, k, D) * (keep != 0).unsqueeze(-1), gx)
    dcls = e["visible_grad_split.dcls"]
    assert torch.allclose(torch.from_numpy(np.asarray(dcls.ref, np.float64)), gcls, rtol=1e-13, atol=1e-13)
    # decoder side: repeat(mask_token) -> scatter(idx_keep, x_decode) -> + decoder_pos_embed  (oracle.forward_decoder)
    xdec, mt, dpos = t64(d["xdec"]).reshape(B, k, D).requires_grad_(), t64(d["mask_token"]).requires_grad_(), t64(d["dpos"])
    dec = torch.scatter(mt.repeat(B, L, 1), 1, keep.unsqueeze(-1).expand(-1, -1, D), xdec) + dpos
    got = t64(e["decoder_assemble.out"].want).reshape(B, L, D)
    assert torch.all((got - dec).abs() <= R.U * dec.abs())
    gxd, gmt = torch.autograd.grad(dec, (xdec, mt), t64(d["dx_dec"]).reshape(B, L, D))
    want = R.from_dt(R.to_dt(gxd.reshape(-1, D).float().numpy(), c.dtype))
    assert np.array_equal(R.bits(R.from_dt(e["decoder_assemble_bwd.d_xdec"].want)), R.bits(want))
    dm = e["decoder_assemble_bwd.d_mask_token"]
    ref = np.zeros(D) if isinstance(dm, R.Exact) else dm.ref
    assert torch.allclose(torch.from_numpy(np.asarray(ref, np.float64)), gmt, rtol=1e-13, atol=1e-13)
    # index maps
    inv = torch.full((B, L), -1, dtype=torch.long).scatter(1, keep, torch.arange(k).expand(B, k))
    assert torch.equal(torch.from_numpy(d["inv"]).long(), inv)
    if k < L:
        assert torch.equal(torch.from_numpy(e["build_row_map.rows"].want).long(), (torch.arange(B).unsqueeze(1) * L + mask).reshape(-1))
        assert sorted(np.concatenate([d["keep"][0], d["mask"][0]]).tolist()) == list(range(L))


@pytest.mark.parametrize("c", SMALL_JEPA, ids=lambda c: c.id)
def test_predictor_references_match_autograd(c):
    d = R.gen_jepa(c)
    e = R.expect_jepa(c, d)
    B, k, nblk, m, D = c.B, c.k, c.nblk, c.m, c.D
    ctx, tgt = torch.from_numpy(d["ctx"]).long(), torch.from_numpy(d["tgt"]).long()
    xdec, mt, pos = t64(d["xdec"]).reshape(B, k, D).requires_grad_(), t64(d["mask_token"]).requires_grad_(), t64(d["pos"])
    seqs = [torch.cat([xdec[b] + pos[ctx[b]], mt + pos[tgt[b, j]]], 0) for b in range(B) for j in range(nblk)]
    out = torch.stack(seqs).reshape(-1, D)
    got = t64(e["predictor_assemble.out"].want)
    assert torch.all((got - out).abs() <= R.U * out.abs())
    gx, gm = torch.autograd.grad(out, (xdec, mt), t64(d["dx"]))
    assert torch.allclose(torch.from_numpy(e["predictor_assemble_bwd.d_xdec"].ref), gx.reshape(-1, D), rtol=1e-13, atol=1e-13)
    assert torch.allclose(torch.from_numpy(e["predictor_assemble_bwd.d_mask_token"].ref), gm, rtol=1e-13, atol=1e-13)
    tail = torch.arange(B * nblk * (k + m)).reshape(B * nblk, k + m)[:, k:].reshape(-1)
    assert torch.equal(torch.from_numpy(e["build_tail_row_map.rows"].want).long(), tail)
    rows = (torch.arange(B).reshape(B, 1, 1) * (c.L - 1) + tgt - 1).reshape(-1)
    assert torch.equal(torch.from_numpy(e["rows_from_tokens.rows"].want).long(), rows)
    assert np.array_equal(R.ref_rows_from_tokens(np.array([[-3, 0, 1, 9, 10, 99]], np.int32), 6, 9), [0, 0, 0, 8, 8, 8])
    assert np.array_equal(R.ref_build_row_map(np.array([[-1, 0, 4, 5]], np.int32), 5), [0, 0, 4, 4])


def test_zero_rows_reference():
    for c in R.zero_cases():
        if c.B * c.T > 4000:
            continue
        d = R.gen_zero(c)
        e = R.expect_zero(c, d)
        a = e["zero_unpredicted_rows.dres"].want.reshape(c.B, c.T, c.D)
        n_clear = int((np.abs(a).sum(-1) == 0).sum())
        assert n_clear == c.B * (c.T - c.m)
        if not c.use_inv:
            assert (a[:, :c.T - c.m] == 0).all() and np.array_equal(a[:, c.T - c.m:], d["dres"].reshape(c.B, c.T, c.D)[:, c.T - c.m:])
        assert R.bits(a).reshape(-1)[0] in (0, R.bits(d["dres"]).reshape(-1)[0])


# ------------------------------------------------------------------------------------------------ the reference inside its bounds
def _all_expectations():
    for c in SMALL_ROWS:
        for exact in (False, True):
            d = R.gen_rows(c, exact)
            yield c.id, R.expect_rows(c, d, exact), R.row_inits(c, d)
    for c in SMALL_JEPA:
        for exact in (False, True):
            d = R.gen_jepa(c, exact)
            yield c.id, R.expect_jepa(c, d, exact), R.jepa_inits(c, d)
    for c in R.zero_cases():
        if c.B * c.T <= 4000:
            d = R.gen_zero(c)
            yield c.id, R.expect_zero(c, d), R.zero_inits(c, d)
    for c in SMALL_PIX:
        d = R.gen_pixels(c, False)
        yield c.id, R.expect_patchify(c, d), R.patchify_inits(c)
        for variant in ("gather", "band"):
            for dp in ("", "f32", "bf16"):
                yield c.id, R.expect_mse(c, d, variant, 1.0 / 3.0, dp), R.loss_inits(c, dp)
    for c in R.gather_cases():
        if not c.lite:
            dg = R.gen_pixels(c, True)
            for dt in ("f32", "bf16"):
                yield c.id, R.expect_gather(c, dg, dt), R.gather_inits(c, dt)
    for c in R.sl1_cases()[:3]:
        d = R.gen_sl1(c)
        for dp in ("", "f32", "bf16"):
            yield c.id, R.expect_sl1(c, d, 1.0, dp), R.sl1_inits(c, dp)


def test_plain_fp32_evaluation_passes_every_checker():
    n = 0
    for cid, e, init in _all_expectations():
        ratios, fails = R.judge(e, R.simulate(e, init), init)
        assert not fails, (cid, fails)
        assert all(r <= 1.0 for r in ratios.values()), (cid, ratios)
        n += 1
    assert n > 300


# ------------------------------------------------------------------------------------------------ mutants
def _rejects(e, init, name, mutate):
    got = R.simulate(e, init)
    assert not R.judge(e, got, init)[1]
    mutate(got[name])
    ratios, fails = R.judge(e, got, init)
    return bool(fails) and not ratios[name] <= 1.0


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("cid", ["D144-tail-f32", "D1024-trip-f32", "D192-GRplus1-f32"])
def test_checker_rejects_a_dropped_or_doubled_row(cid, exact):
    c = next(x for x in R.row_cases() if x.id == cid)
    d = R.gen_rows(c, exact)
    e, init = R.expect_rows(c, d, exact), R.row_inits(c, d)
    masked = d["dx_dec"][(d["inv"] < 0).reshape(-1)]
    cls_rows = d["dx_vis"][d["keep"].reshape(-1) == 0]
    for name, rows in (("decoder_assemble_bwd.d_mask_token", masked), ("visible_grad_split.dcls", cls_rows)):
        row = rows[len(rows) // 2]
        col = int(np.argmax(np.abs(row)))
        if exact and row[col] == 0:
            continue
        for sign in (-1.0, 1.0):      # dropped, doubled: the column where that row is largest must leave the bound
            def mutate(buf, sign=sign, row=row):
                buf[:c.D] = (buf[:c.D].astype(np.float64) + sign * row).astype(np.float32)
            got = R.simulate(e, init)
            mutate(got[name])
            ratios, fails = R.judge(e, got, init)
            if exact:
                assert fails and ratios[name] == np.inf
            else:                        # a random row is far above c u sum|x| unless the sum is over very many rows
                assert fails and ratios[name] > 1.0


def test_checker_rejects_index_order_ulp_guard_and_untouched_mutants():
    c = next(x for x in R.row_cases() if x.id == "D192-GRplus1-bf16")
    d = R.gen_rows(c)
    e, init = R.expect_rows(c, d), R.row_inits(c, d)

    def off_by_one_token(buf):         # assemble_visible with pos[t + 1] on one row
        t = d["keep"].reshape(-1)
        buf[2] = np.where(t[2] == 0, d["cls"], d["x"][2]) + d["pos"][(t[2] + 1) % c.L]
    assert _rejects(e, init, "assemble_visible.x", off_by_one_token)

    def one_bf16_ulp(buf):
        buf[1, 3] += 1
    assert _rejects(e, init, "visible_grad_split.dtok", one_bf16_ulp)
    assert _rejects(e, init, "decoder_assemble_bwd.d_xdec", one_bf16_ulp)

    def guard_row(buf):
        buf[c.dec_rows] = 0.0
    assert _rejects(e, init, "decoder_assemble.out", guard_row)

    def guard_of_sum(buf):
        buf[c.D] = 0.0
    assert _rejects(e, init, "visible_grad_split.dcls", guard_of_sum)

    def behind_scratch(buf):
        buf[R.PARTIAL_BLOCKS * c.D] = 0.0
    assert _rejects(e, init, "visible_grad_split.partial", behind_scratch)

    def inv_off_by_one(buf):
        buf[5] += 1
    assert _rejects(e, init, "build_inverse.inv", inv_off_by_one)
    assert _rejects(e, init, "build_row_map.rows", inv_off_by_one)

    def nan_to_number(buf):            # a class-token row of dtok left as it was
        buf[0] = init["visible_grad_split.dtok"][0]
    assert d["keep"][0, 0] == 0 and _rejects(e, init, "visible_grad_split.dtok", nan_to_number)

    z = next(x for x in R.zero_cases() if x.id == "D264-tail-m1")
    dz = R.gen_zero(z)
    ez, iz = R.expect_zero(z, dz), R.zero_inits(z, dz)

    def untouched_row(buf):
        buf[z.T - 1, 7] = 0
    assert _rejects(ez, iz, "zero_unpredicted_rows.dres", untouched_row) and _rejects(ez, iz, "zero_unpredicted_rows.dres_c", untouched_row)

    def stale_row(buf):
        buf[0, z.D // 4 - 1] = 1.0     # the last float4 of a row that should be zero
    assert _rejects(ez, iz, "zero_unpredicted_rows.dres", stale_row)

    p = next(x for x in R.loss_cases() if x.id == "c3i32p8-oor")
    dp = R.gen_pixels(p, False)
    ep, ip = R.expect_mse(p, dp, "band", 1.0, "f32"), R.loss_inits(p, "f32")
    pat = R.patches_of(dp["f32"][:p.B], p.p, "cpp")     # the element order of the other gather: (c, py, px)

    def wrong_order(buf):
        t = pat[0, np.clip(dp["tok"][0, 2] - 1, 0, p.g ** 2 - 1)]
        buf[2] = (dp["pred"][2] - t) * R.mse_gs(1.0, dp["pred"].size)
    assert _rejects(ep, ip, "mse.d_pred", wrong_order)

    def no_upper_clamp(buf):           # id g*g + 1 read as patch g*g: the rows below the image = the next channel / the spare image
        buf[1] = np.nan
    assert dp["tok"][0, 1] == p.g ** 2 + 1 and _rejects(ep, ip, "mse.d_pred", no_upper_clamp)

    def loss_off(buf):
        buf[0] *= np.float32(1 + 1e-4)
    assert _rejects(ep, ip, "mse.loss", loss_off)
    q = next(x for x in R.gather_cases() if x.id == "c3i32p8-all")
    g = R.gen_pixels(q, True)
    eg, ig = R.expect_gather(q, g, "f32"), R.gather_inits(q, "f32")
    j = int(np.argmax(g["tok"][0] > 0))

    def ppc_for_cpp(buf):
        buf[j] = R.patches_of(g["f32"][:q.B], q.p, "ppc")[0, g["tok"][0, j] - 1]
    assert _rejects(eg, ig, "gather_patches.out", ppc_for_cpp)

    def neighbour_patch(buf):
        buf[j] = R.patches_of(g["f32"][:q.B], q.p, "cpp")[0, g["tok"][0, j] % (q.g ** 2)]
    assert _rejects(eg, ig, "gather_patches.out", neighbour_patch)
