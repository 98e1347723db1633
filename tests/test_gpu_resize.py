"""mae_resize_crop_flip (k_resize.hip) on the MI355X against the fp64 reference of tests/resize_ref.py, per pixel: every case
of its table (non-integer and integer ratios both ways, a small odd output, the two store tails, the workload's 96 -> 224 and
the same size) under every box set (whole image, flips, 1 x 1 boxes, boxes on each border, one-column / one-row boxes, seeded
RandomResizedCrop draws), all three dtype routes; the bit-for-bit properties; every refusal; one out-of-image box at the C level."""
import numpy as np
import pytest
import torch

from tests import resize_ref as R
from tests.util import stream

pytestmark = pytest.mark.gpu

F32, U8 = 0, 2
IDS = ["x".join(map(str, c)) for c in R.CASES]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def sentinel(dev, B, C, So, out_dt):
    """A value in every element that the kernel cannot produce by leaving it alone: NaN, or byte 201 behind a written mask."""
    return torch.full((B, C, So, So), 201, dtype=torch.uint8, device=dev) if out_dt == U8 else torch.full((B, C, So, So), float("nan"), device=dev)


def call_resize(dev, images, params, So, out_dt, out=None, check_rc=True):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    x = (images if torch.is_tensor(images) else torch.from_numpy(np.array(images))).to(dev)
    B, C, Si, _ = x.shape
    in_dt = U8 if x.dtype == torch.uint8 else F32
    p = None if params is None else torch.as_tensor(np.asarray(params), dtype=torch.int32).to(dev).contiguous()
    if out is None:
        out = sentinel(dev, B, C, So, out_dt)
    rc = lib.mae_resize_crop_flip(_ptr(x), in_dt, B, C, Si, _ptr(p), So, out_dt, _ptr(out), stream(dev))
    if not check_rc:
        check(0)
        return rc
    check(rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_every_route_within_the_bound(dev, case):
    from ssrl_vit_mae_jepa_amd.data import normalize_u8
    B, C, Si, So = case
    u8, f32 = R.inputs(B, C, Si)
    for name, params in R.box_sets(B, Si):
        ref, delta = R.reference(case, name, params, "u8")
        o8 = call_resize(dev, u8, params, So, U8)
        err = np.abs(o8.astype(np.float64) - ref)
        worst = float((err / (0.5 + delta)).max())
        print(f"{case} {name} u8->u8 : worst |out - ref| {float(err.max()):.6f}, bound 0.5 + {float(delta.max()):.3e}, worst ratio {worst:.4f}")
        assert worst <= 1.0, (case, name)
        o8f = call_resize(dev, u8, params, So, F32)
        assert np.isfinite(o8f).all(), "an output pixel was not written"
        assert np.array_equal(o8f.view(np.uint32), normalize_u8(torch.from_numpy(o8)).numpy().view(np.uint32)), (case, name, "u8->f32 is not normalize_u8 of u8->u8")
        reff, deltaf = R.reference(case, name, params, "f32")
        of = call_resize(dev, f32, params, So, F32)
        assert np.isfinite(of).all(), "an output pixel was not written"
        errf = np.abs(of.astype(np.float64) - reff)
        worstf = float((errf / deltaf).max())
        print(f"{case} {name} f32->f32: worst |out - ref| {float(errf.max()):.3e}, bound {float(deltaf.max()):.3e}, worst ratio {worstf:.4f}")
        assert worstf <= 1.0, (case, name)


@pytest.mark.parametrize("case", R.CASES, ids=IDS)
def test_bit_for_bit_properties(dev, case):
    B, C, Si, So = case
    u8, f32 = R.inputs(B, C, Si)
    sets = dict(R.box_sets(B, Si))
    for x, out_dt in ((u8, U8), (u8, F32), (f32, F32)):
        # NULL params = explicit whole-image rows
        a = call_resize(dev, x, None, So, out_dt)
        b = call_resize(dev, x, R.whole(B, Si), So, out_dt)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
        # a flip of the whole image is the mirror of the unflipped result (the taps are the same integers)
        fl = call_resize(dev, x, R.whole(B, Si, 1), So, out_dt)
        assert np.array_equal(fl, a[..., ::-1])
        for name in ("rrc08", "borders0", "column"):
            p = sets[name]
            full = call_resize(dev, x, p, So, out_dt)
            again = call_resize(dev, x, p, So, out_dt)
            assert np.array_equal(full.view(np.uint8), again.view(np.uint8)), "a second run differs"
            for i in range(B):   # image i alone = image i of the batch
                alone = call_resize(dev, x[i:i + 1], p[i:i + 1], So, out_dt)
                assert np.array_equal(alone.view(np.uint8), full[i:i + 1].view(np.uint8)), (name, i)
    # a byte batch off the 4-byte grid is read tap by tap instead of through aligned 8-byte windows: the same bytes come out
    buf = torch.empty(u8.size + 1, dtype=torch.uint8, device=dev)
    odd = buf[1:].view(u8.shape)
    odd.copy_(torch.from_numpy(u8.copy()))
    for name in ("whole", "rrc08", "borders0"):
        for out_dt in (U8, F32):
            assert np.array_equal(call_resize(dev, odd, sets[name], So, out_dt).view(np.uint8), call_resize(dev, u8, sets[name], So, out_dt).view(np.uint8)), name
    if Si == So:   # identity and flip-only copy the source, bytes and floats
        assert np.array_equal(call_resize(dev, u8, R.whole(B, Si), So, U8), u8)
        assert np.array_equal(call_resize(dev, u8, R.whole(B, Si, 1), So, U8), u8[..., ::-1])
        assert np.array_equal(call_resize(dev, f32, R.whole(B, Si), So, F32).view(np.uint32), f32.view(np.uint32))
        assert np.array_equal(call_resize(dev, f32, R.whole(B, Si, 1), So, F32).view(np.uint32), np.ascontiguousarray(f32[..., ::-1]).view(np.uint32))


def test_refusals_before_launch(dev):
    from ssrl_vit_mae_jepa_amd._lib import lib
    B, C, Si, So = 2, 3, 8, 18
    u8, f32 = R.inputs(B, C, Si)
    xu, xf = torch.from_numpy(u8.copy()).to(dev), torch.from_numpy(f32.copy()).to(dev)
    s = stream(dev)

    def refused(word, x, in_dt, b, c, si, so, out_dt, out=None, null_in=False, null_out=False):
        guard = sentinel(dev, B, C, So, U8 if out_dt == U8 else F32) if out is None else out
        before = guard.clone()
        rc = lib.mae_resize_crop_flip(None if null_in else x.data_ptr(), in_dt, b, c, si, None, so, out_dt, None if null_out else guard.data_ptr(), s)
        assert rc != 0 and word in lib.mae_last_error(), (word, lib.mae_last_error())
        torch.cuda.synchronize()
        assert torch.equal(guard.view(torch.uint8), before.view(torch.uint8)), f"{word}: out was written"

    refused(b"null", xu, U8, B, C, Si, So, U8, null_in=True)
    refused(b"null", xu, U8, B, C, Si, So, U8, null_out=True)
    for b, c, si, so in ((0, C, Si, So), (-1, C, Si, So), (B, 0, Si, So), (B, C, 0, So), (B, C, Si, 0), (B, C, Si, -4)):
        refused(b"bad batch", xu, U8, b, c, si, so, U8)
    refused(b"<= 8192", xu, U8, 1, 1, 8, 8193, U8)
    # in_size > 8 * out_size: the buffers would be large enough (only the check is reached)
    big = torch.zeros(1, 1, 18, 18, dtype=torch.uint8, device=dev)
    refused(b"tap count", big, U8, 1, 1, 18, 2, U8)
    for bad in (1, 3, -1):   # bf16 / unknown dtypes, either side
        refused(b"in_dtype", xu, bad, B, C, Si, So, U8)
        refused(b"out_dtype", xu, U8, B, C, Si, So, bad)
    refused(b"uint8 output needs uint8", xf, F32, B, C, Si, So, U8)
    # out overlapping images: the same buffer, and a partial overlap
    same = torch.zeros(B * C * So * So, dtype=torch.uint8, device=dev)
    refused(b"overlap", same, U8, B, C, Si, So, U8, out=same)
    refused(b"overlap", same[16:], U8, B, C, Si, So, U8, out=same)
    fbuf = torch.zeros(B * C * So * So + 64, device=dev)
    refused(b"overlap", fbuf[32:], F32, B, C, Si, So, F32, out=fbuf)
    # a float buffer off the 4-byte grid
    raw = torch.zeros(4 * B * C * So * So + 8, dtype=torch.uint8, device=dev)
    rc = lib.mae_resize_crop_flip(xu.data_ptr(), U8, B, C, Si, None, So, F32, raw.data_ptr() + 1, s)
    assert rc != 0 and b"aligned" in lib.mae_last_error()
    torch.cuda.synchronize()
    assert bool((raw == 0).all())


def test_wrapper(dev):
    """data.resize_batch: dtypes in and out, tuple / tensor / device parameters, the ValueErrors."""
    from ssrl_vit_mae_jepa_amd.data import draw_augment_params, normalize_u8, resize_batch
    B, C, Si, So = 3, 3, 96, 112
    u8, f32 = R.inputs(B, C, Si)
    xu, xf = torch.from_numpy(u8.copy()).to(dev), torch.from_numpy(f32.copy()).to(dev)
    plain = resize_batch(xu, So)
    assert plain.dtype == torch.uint8 and tuple(plain.shape) == (B, C, So, So)
    assert np.array_equal(plain.cpu().numpy(), call_resize(dev, u8, None, So, U8))
    assert torch.equal(resize_batch(xu, So, out_dtype=torch.float32).cpu(), normalize_u8(plain.cpu()))   # the host expression: IEEE division
    assert resize_batch(xf, So).dtype == torch.float32
    g = torch.Generator(device=dev).manual_seed(5)
    draw = draw_augment_params(B, Si, g)
    rows = torch.stack([t.to(torch.int64) for t in draw], dim=1)
    a = resize_batch(xu, So, params=draw)
    assert torch.equal(a, resize_batch(xu, So, params=rows)) and torch.equal(a, resize_batch(xu, So, params=rows.cpu()))
    assert np.array_equal(a.cpu().numpy(), call_resize(dev, u8, rows.cpu().numpy(), So, U8))
    assert resize_batch(xu[:0], So).shape == (0, C, So, So)
    with pytest.raises(ValueError, match="does not lie inside"):
        resize_batch(xu, So, params=torch.tensor([[0, 0, 96, 96, 0], [1, 0, 96, 96, 0], [0, 0, 96, 96, 0]]))
    with pytest.raises(ValueError):
        resize_batch(xu[:, :, :, :90], So)          # not square
    with pytest.raises(ValueError):
        resize_batch(xu.cpu(), So)                  # not on the device
    with pytest.raises(ValueError):
        resize_batch(xu.to(torch.int32), So)        # a dtype the kernel does not read
    with pytest.raises(ValueError):
        resize_batch(xf, So, out_dtype=torch.uint8)
    with pytest.raises(ValueError):
        resize_batch(xu, 11)                        # 96 > 8 * 11
    with pytest.raises(ValueError):
        resize_batch(xu, So, params=rows[:2])


def test_box_outside_the_image_is_clamped(dev):
    """The boxes are device data the launcher cannot check: the kernel clamps them and every tap index, so a box far outside
    the image gives finite, in-range pixels (one call; the wrapper refuses such a box on the host)."""
    So = 7
    u8, _ = R.inputs(2, 4, 12)
    x8 = np.ascontiguousarray(np.tile(u8[:, :3], (2, 1, 1, 1)))   # (4, 3, 12, 12)
    wild = np.array([[-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1, -5, 1], [10 ** 6, -10 ** 6, 10 ** 6, 10 ** 6, 0], [5, 40, 0, 3, 7], [-3, -3, 40, 40, 1]],
                    dtype=np.int64).astype(np.int32)
    out = call_resize(dev, x8, wild, So, F32)   # the sentinel is NaN: every pixel was written, with a normalised byte of the image
    assert np.isfinite(out).all() and out.min() >= -1.0 and out.max() <= 1.0
    lo, hi = (x8.min() / 255.0 - 0.5) / 0.5, (x8.max() / 255.0 - 0.5) / 0.5
    assert out.min() >= lo - 1e-6 and out.max() <= hi + 1e-6   # convex weights: inside the image's range
