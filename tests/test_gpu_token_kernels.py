"""The kernels that move tokens and pixels between the GEMMs, and the losses that read the image (k_patch.hip, k_pixels.hip,
k_index.hip, k_jepa.hip), one by one through the C ABI against tests/token_ref.py (-m gpu).

Every case of token_ref's tables.  Copies, single fp32 additions, bf16 roundings, zeros, index maps and d_pred are compared bit
for bit; column sums are bit-exact on the integer inputs and inside c u sum|x| on random ones; loss scalars inside
(c + 3) u ref (token_ref's docstring counts c from the code).  Every output buffer starts NaN-filled (or holds a pattern) with
guard rows behind it and is compared as a whole, so nothing outside the specified rows may change; two launches into separate
buffers must agree bit for bit.  Every kernel gets the reference's index maps, not another kernel's output, so each is judged
on its own.  The last test prints the worst error / bound per kernel and output.

The whole file (200 tests) takes about 6 s on an MI355X; the largest case (82 070 rows of 192) 0.35 s."""
import re

import numpy as np
import pytest
import torch

from ssrl_vit_mae_jepa_amd._lib import MaeHipError
from tests import token_ref as R
from tests.util import _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1, "u8": 2, "": 0}   # MAE_F32, MAE_BF16, MAE_U8
ROWS = {c.id: c for c in R.row_cases()}
ZEROS = {c.id: c for c in R.zero_cases()}
JEPA = {c.id: c for c in R.jepa_cases()}
GATHER = {c.id: c for c in R.gather_cases()}
LOSS = {c.id: c for c in R.loss_cases()}
SL1 = {c.id: c for c in R.sl1_cases()}
DPRED_FULL = [(dp, gs) for dp in ("", "f32", "bf16") for gs in (1.0, 1.0 / 3.0)]
DPRED_LITE = [("", 1.0), ("f32", 1.0 / 3.0), ("bf16", 1.0)]
WORST = {}   # (kernel.output, variant) -> (worst error / bound, case id)


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def up(a, dev):
    """A numpy buffer on the device, bit for bit (bf16 patterns travel as int16)."""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def down(t, like):
    return t.cpu().numpy().view(like.dtype).reshape(like.shape)


def run_twice(init, launch, dev, what):
    """launch(buffers) into two separate sets of buffers loaded with init -> the first set on the host; both must agree bit for bit."""
    sets = []
    for _ in range(2):
        bufs = {k: up(v, dev) for k, v in init.items()}
        launch(bufs)
        sets.append(bufs)
    torch.cuda.synchronize()
    for k in init:
        a, b = (v.view(torch.int32) if v.dtype == torch.float32 else v for v in (sets[0][k], sets[1][k]))   # bits: NaN guards compare equal
        assert torch.equal(a, b), f"{what}: two launches differ in {k}"
    return {k: down(v, init[k]) for k, v in sets[0].items()}


def settle(cid, variant, e, got, init, fails_out):
    ratios, fails = R.judge(e, got, init)
    for k, v in ratios.items():
        if (k, variant) not in WORST or v > WORST[(k, variant)][0]:
            WORST[(k, variant)] = (v, cid)
    print(cid, variant, {k: f"{v:.3f}" for k, v in ratios.items() if not isinstance(e[k], R.Exact)})
    fails_out += [f"{cid} [{variant}] {f}" for f in fails]


def rejected(call, init, message, dev):
    """The call returns non-zero with the documented message and writes nothing."""
    bufs = {k: up(v, dev) for k, v in init.items()}
    with pytest.raises(MaeHipError, match=re.escape(message)):
        check(call(bufs))
    torch.cuda.synchronize()
    return all(np.array_equal(R.bits(down(bufs[k], init[k])), R.bits(init[k])) for k in init)


# ------------------------------------------------------------------------------------------------ MAE rows
@pytest.mark.parametrize("cid", list(ROWS))
def test_mae_row_kernels(dev, cid):
    c, s, fails = ROWS[cid], stream(dev), []
    for exact in ((False,) if "grid2" in cid else (False, True)):
        d = R.gen_rows(c, exact)
        init, e = R.row_inits(c, d), R.expect_rows(c, d, exact)
        t = {k: up(d[k], dev) for k in ("keep", "mask", "inv", "cls", "pos", "dx_vis", "xdec", "mask_token", "dpos", "dx_dec")}
        dt = DT[c.dtype]

        def launch(b):
            check(lib.mae_build_inverse(_ptr(t["keep"]), c.B, c.k, c.L, _ptr(b["build_inverse.inv"]), s))
            if c.k < c.L:
                check(lib.mae_build_row_map(_ptr(t["mask"]), c.B, c.L - c.k, c.L, _ptr(b["build_row_map.rows"]), s))
            check(lib.mae_assemble_visible(_ptr(b["assemble_visible.x"]), _ptr(t["keep"]), _ptr(t["cls"]), _ptr(t["pos"]), c.vis_rows, c.D, s))
            check(lib.mae_visible_grad_split(_ptr(t["dx_vis"]), _ptr(t["keep"]), c.vis_rows, c.D, dt, _ptr(b["visible_grad_split.dtok"]),
                                             _ptr(b["visible_grad_split.dcls"]), _ptr(b["visible_grad_split.partial"]), s))
            check(lib.mae_decoder_assemble(_ptr(t["xdec"]), dt, _ptr(t["inv"]), _ptr(t["mask_token"]), _ptr(t["dpos"]), c.B, c.k, c.L, c.D,
                                           _ptr(b["decoder_assemble.out"]), s))
            check(lib.mae_decoder_assemble_bwd(_ptr(t["dx_dec"]), _ptr(t["inv"]), c.B, c.k, c.L, c.D, dt, _ptr(b["decoder_assemble_bwd.d_xdec"]),
                                               _ptr(b["decoder_assemble_bwd.d_mask_token"]), _ptr(b["decoder_assemble_bwd.partial"]), s))

        got = run_twice(init, launch, dev, cid)
        settle(cid, c.dtype + (" integers" if exact else ""), e, got, init, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", list(ZEROS))
def test_zero_unpredicted_rows(dev, cid):
    c, s, fails = ZEROS[cid], stream(dev), []
    d = R.gen_zero(c)
    init, e = R.zero_inits(c, d), R.expect_zero(c, d)
    inv = up(d["inv"], dev)

    def launch(b):
        check(lib.mae_zero_unpredicted_rows(_ptr(inv), c.B * c.T, c.T, c.m, c.D, DT[c.dtype], _ptr(b["zero_unpredicted_rows.dres"]),
                                            _ptr(b["zero_unpredicted_rows.dres_c"]), s))

    settle(cid, c.dtype, e, run_twice(init, launch, dev, cid), init, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ I-JEPA rows
@pytest.mark.parametrize("cid", list(JEPA))
def test_predictor_row_kernels(dev, cid):
    c, s, fails = JEPA[cid], stream(dev), []
    for exact in (False, True):
        d = R.gen_jepa(c, exact)
        init, e = R.jepa_inits(c, d), R.expect_jepa(c, d, exact)
        t = {k: up(d[k], dev) for k in ("ctx", "tgt", "xdec", "mask_token", "pos", "dx")}
        dt = DT[c.dtype]

        def launch(b):
            check(lib.mae_predictor_assemble(_ptr(t["xdec"]), dt, _ptr(t["ctx"]), _ptr(t["tgt"]), _ptr(t["mask_token"]), _ptr(t["pos"]), c.B, c.k,
                                             c.nblk, c.m, c.L, c.D, _ptr(b["predictor_assemble.out"]), s))
            check(lib.mae_predictor_assemble_bwd(_ptr(t["dx"]), c.B, c.k, c.nblk, c.m, c.D, dt, _ptr(b["predictor_assemble_bwd.d_xdec"]),
                                                 _ptr(b["predictor_assemble_bwd.d_mask_token"]), _ptr(b["predictor_assemble_bwd.partial"]), s))
            check(lib.mae_build_tail_row_map(c.B * c.nblk, c.k + c.m, c.m, _ptr(b["build_tail_row_map.rows"]), s))
            check(lib.mae_rows_from_tokens(_ptr(t["tgt"]), c.B, c.nblk * c.m, c.L - 1, _ptr(b["rows_from_tokens.rows"]), s))

        settle(cid, c.dtype + (" integers" if exact else ""), e, run_twice(init, launch, dev, cid), init, fails)
    assert not fails, "\n".join(fails)


def test_index_kernels_past_their_grids(dev):
    """More than 2048 * 256 elements: the grid-stride second trip; ids outside the range are clamped, never used as they are."""
    s, fails, rng = stream(dev), [], np.random.default_rng(5)
    for name, a in R.INDEX_TRIPS:
        if name == "build_row_map":
            idx = rng.integers(-1, a["L"] + 1, size=(a["B"], a["n_per"])).astype(np.int32)
            want, t = R.ref_build_row_map(idx, a["L"]), up(idx, dev)
            call = lambda b: check(lib.mae_build_row_map(_ptr(t), a["B"], a["n_per"], a["L"], _ptr(b[key]), s))
        elif name == "build_tail_row_map":
            want = R.ref_tail_row_map(a["seqs"], a["T"], a["m"])
            call = lambda b: check(lib.mae_build_tail_row_map(a["seqs"], a["T"], a["m"], _ptr(b[key]), s))
        else:
            tok = rng.integers(-1, a["N"] + 3, size=(a["B"], a["per_image"])).astype(np.int32)
            want, t = R.ref_rows_from_tokens(tok, a["per_image"], a["N"]), up(tok, dev)
            call = lambda b: check(lib.mae_rows_from_tokens(_ptr(t), a["B"], a["per_image"], a["N"], _ptr(b[key]), s))
        key = f"{name}.rows"
        init, e = {key: R.nan_buf(want.size, 0, "i32")}, {key: R.Exact(want)}
        settle(name, "second trip", e, run_twice(init, call, dev, name), init, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------ pixels
@pytest.mark.parametrize("cid", list(GATHER))
def test_gather_patches(dev, cid):
    c, s, fails = GATHER[cid], stream(dev), []
    d = R.gen_pixels(c, True)
    images, tok = {"f32": up(d["f32"], dev), "u8": up(d["u8"], dev)}, up(d["tok"], dev)
    for image_dtype in ("f32", "u8"):
        for out_dtype in ("f32", "bf16"):
            init = R.gather_inits(c, out_dtype)

            def launch(b):
                return lib.mae_gather_patches(_ptr(images[image_dtype]), DT[image_dtype], _ptr(tok), c.B, c.n, c.C, c.img, c.p, DT[out_dtype],
                                              _ptr(b["gather_patches.out"]), s)

            if image_dtype == "u8" and not R.u8_supported(c.C, c.img, c.p, c.n):
                assert rejected(launch, init, R.U8_GATHER_MESSAGE, dev), f"{cid}: a rejected geometry wrote to its output"
                continue
            got = run_twice(init, lambda b: check(launch(b)), dev, cid)
            settle(cid, f"{image_dtype} -> {out_dtype}", R.expect_gather(c, d, out_dtype), got, init, fails)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", list(LOSS))
def test_mse_loss_from_images(dev, cid):
    """The three variants on the same token list: the engine's path for float images (band walk where it applies), the per-pixel
    gather (path 1) and the uint8 band walk.  Ids 0 and g*g + 1 (kind oor) must read patches 0 and g*g - 1 in all of them: the
    image behind the batch is NaN / 255, so a missing clamp shows up as a wrong value."""
    c, s, fails = LOSS[cid], stream(dev), []
    d = R.gen_pixels(c, False)
    images, tok, pred = {"f32": up(d["f32"], dev), "u8": up(d["u8"], dev)}, up(d["tok"], dev), up(d["pred"], dev)
    seen = {}
    for image_dtype, path in (("f32", 0), ("f32", 1), ("u8", 0)):
        for dp, gs in (DPRED_LITE if c.lite else DPRED_FULL):
            init = R.loss_inits(c, dp)

            def launch(b):
                return lib.mae_mse_loss_from_images(_ptr(pred), _ptr(images[image_dtype]), DT[image_dtype], _ptr(tok), c.B, c.n, c.C, c.img, c.p, gs,
                                                    _ptr(b["mse.loss"]), _ptr(b["mse.d_pred"]) if dp else None, DT[dp], _ptr(b["mse.scratch"]),
                                                    path, s)

            if image_dtype == "u8" and not R.u8_supported(c.C, c.img, c.p, c.n):
                assert rejected(launch, init, R.U8_LOSS_MESSAGE, dev), f"{cid}: a rejected geometry wrote to its outputs"
                continue
            variant = R.mse_variant(c, image_dtype, path)
            e = R.expect_mse(c, d, variant, gs, dp)
            got = run_twice(init, lambda b: check(launch(b)), dev, cid)
            settle(cid, f"{image_dtype} {variant}", e, got, init, fails)
            seen[(image_dtype, path, dp, gs)] = (got, e["mse.loss"])
    if R.band_f32_eligible(c.C, c.img, c.p, c.n):     # path 0 took the band walk here: the gather must agree with it
        for (image_dtype, path, dp, gs), (got, exp) in seen.items():
            if image_dtype == "f32" and path == 1:
                other, oexp = seen[("f32", 0, dp, gs)]
                if dp:
                    assert np.array_equal(R.bits(got["mse.d_pred"]), R.bits(other["mse.d_pred"])), f"{cid}: d_pred of the two float variants differ"
                assert abs(float(got["mse.loss"][0]) - float(other["mse.loss"][0])) <= exp.bound[0] + oexp.bound[0]
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("cid", list(LOSS))
def test_patchify_gather(dev, cid):
    """The target the loss never materialises, on the loss's token lists (ids as int64, as the ABI takes them): ids 0 and g*g + 1
    (kind oor) copy patches 0 and g*g - 1 from either image dtype."""
    c, s, fails = LOSS[cid], stream(dev), []
    d = R.gen_pixels(c, False)
    images, idx = {"f32": up(d["f32"], dev), "u8": up(d["u8"], dev)}, up(d["tok"].astype(np.int64), dev)
    init, e = R.patchify_inits(c), R.expect_patchify(c, d)
    for image_dtype in ("f32", "u8"):
        def launch(b):
            return lib.mae_patchify_gather(_ptr(images[image_dtype]), DT[image_dtype], _ptr(idx), c.B, c.C, c.img, c.p, c.n,
                                           _ptr(b["patchify_gather.target"]), s)

        if image_dtype == "u8" and not R.u8_supported(c.C, c.img, c.p, c.n):
            assert rejected(launch, init, R.U8_LOSS_MESSAGE, dev), f"{cid}: a rejected geometry wrote to its output"
            continue
        settle(cid, image_dtype, e, run_twice(init, lambda b: check(launch(b)), dev, cid), init, fails)
    assert not fails, "\n".join(fails)


def test_loss_wrapper_rejects_what_it_cannot_run(dev):
    c = LOSS["c3i32p8-random"]
    d = R.gen_pixels(c, False)
    u8, tok, pred, s = up(d["u8"], dev), up(d["tok"], dev), up(d["pred"], dev), stream(dev)
    init = R.loss_inits(c, "f32")
    for image_dtype, path, message in ((DT["u8"], 1, "path must be 0, or 1 with MAE_F32 images"), (DT["f32"], 2, "path must be 0"), (1, 0, "image_dtype must be")):
        def call(b):
            return lib.mae_mse_loss_from_images(_ptr(pred), _ptr(u8), image_dtype, _ptr(tok), c.B, c.n, c.C, c.img, c.p, 1.0, _ptr(b["mse.loss"]),
                                                _ptr(b["mse.d_pred"]), 0, _ptr(b["mse.scratch"]), path, s)
        assert rejected(call, init, message, dev)


# ------------------------------------------------------------------------------------------------ smooth L1
@pytest.mark.parametrize("cid", list(SL1))
def test_smooth_l1(dev, cid):
    c, s, fails = SL1[cid], stream(dev), []
    d = R.gen_sl1(c)
    pred, target = up(d["pred"], dev), up(d["target"], dev)
    for dp, gs in DPRED_FULL:
        init, e = R.sl1_inits(c, dp), R.expect_sl1(c, d, gs, dp)

        def launch(b):
            check(lib.mae_smooth_l1_loss(_ptr(pred), _ptr(target), c.n, gs, _ptr(b["smooth_l1.loss"]), _ptr(b["smooth_l1.d_pred"]) if dp else None,
                                         DT[dp], _ptr(b["smooth_l1.scratch"]), s))

        settle(cid, "", e, run_twice(init, launch, dev, cid), init, fails)
    assert not fails, "\n".join(fails)


def test_zz_report():
    """Prints the worst error / bound per kernel output and variant over the cases that ran (0 = bit-exact everywhere)."""
    print("\nworst error / bound per output and variant:")
    for (k, variant), (ratio, cid) in sorted(WORST.items()):
        print(f"  {k:40s} {variant:24s} {ratio:.3f}  ({cid})")
    assert WORST and all(v[0] <= 1.0 for v in WORST.values())
