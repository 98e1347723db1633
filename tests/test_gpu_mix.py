"""mae_mix_batch (k_mix.hip) on the MI355X against the fp64 reference of tests/mix_ref.py, per element: both input and both
output dtypes, every vector width (S = 8 and 12: 4 pixels per thread, S = 96: 16 with uint8 output, 4 with fp32; S = 7: single pixels),
box edges off the vector grid, empty / full / over-range boxes, lam in {0, 0.37, 1}, an out-of-range partner, and the
rejections that happen before any launch."""
import numpy as np
import pytest
import torch

from tests import mix_ref as R
from tests.util import stream

pytestmark = pytest.mark.gpu

F32, U8 = 0, 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def call_mix(dev, images, partner, lam, box, out_dt, out=None, check_rc=True):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    B, C, S, _ = images.shape
    x = images if images.is_cuda else images.to(dev)
    in_dt = U8 if x.dtype == torch.uint8 else F32
    p = torch.as_tensor(partner, dtype=torch.int32).to(dev)
    l = torch.as_tensor(lam, dtype=torch.float32).to(dev) if lam is not None else None
    bx = torch.as_tensor(box, dtype=torch.int32).to(dev).contiguous()
    if out is None:  # a sentinel in every byte: each one must be written
        out = torch.full((B, C, S, S), 201, dtype=torch.uint8, device=dev) if out_dt == U8 else torch.full((B, C, S, S), float("nan"), device=dev)
    rc = lib.mae_mix_batch(_ptr(x), in_dt, _ptr(p), _ptr(l), _ptr(bx), B, C, S, out_dt, _ptr(out), stream(dev))
    if not check_rc:
        check(0)
        return rc
    check(rc)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def boxes(B, S, first=0):
    """Per image, starting at case ``first``: edges off the 4-pixel grid, an empty box, the full image, an over-range box whose
    left edge lies off the 16-pixel grid in mid-row, a one-pixel box."""
    cases = [(1, S - 1, 1, min(7, S)), (3, 3, 0, S), (0, S, 0, S), (-5, S + 9, S // 2 + 1, 4 * S), (S - 1, S, S - 1, S)]
    return [cases[(first + b) % len(cases)] for b in range(B)]


def box_sets(B, S):
    """Every box case reaches every shape: a batch shorter than the case list is run again from where the first set stopped."""
    return [boxes(B, S)] if B >= 5 else [boxes(B, S), boxes(B, S, first=B)]


CASES = [(5, 3, 8), (5, 3, 12), (3, 3, 96), (5, 2, 7)]
_inputs = {}


def inputs(B, C, S):
    if (B, C, S) not in _inputs:
        g = np.random.default_rng(B * 1000 + C * 100 + S)
        u8 = g.integers(0, 256, (B, C, S, S), dtype=np.uint8)
        u8.reshape(-1)[:2] = (0, 255)
        f32 = (g.standard_normal((B, C, S, S)) * 1.5).astype(np.float32)
        _inputs[(B, C, S)] = (u8, f32)
    return _inputs[(B, C, S)]


def compare_f32(out, images, partner, lam, box, what):
    ref, bound, exact = R.mix_reference(images, partner, lam, box)
    assert np.isfinite(out).all(), f"{what}: an output pixel was not written"
    n = R.normalize_u8_f32(images) if images.dtype == np.uint8 else images
    B = images.shape[0]
    inside = np.broadcast_to(R.inside_mask(box, images.shape[-1])[:, None], out.shape)
    want_exact = np.where(inside, n[R.effective_partner(partner, B)], n)
    assert np.array_equal(out[exact].view(np.uint32), want_exact[exact].view(np.uint32)), f"{what}: a copied pixel is not bit-exact"
    err = np.abs(out.astype(np.float64) - ref)
    blend = ~exact
    worst = float((err[blend] / bound[blend]).max()) if blend.any() else 0.0
    print(f"{what}: {int(exact.sum())} exact pixels, {int(blend.sum())} blended, worst error / bound {worst:.3f}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("B,C,S", CASES)
@pytest.mark.parametrize("in_dt", [U8, F32])
def test_mix_f32_output_matches_reference(dev, B, C, S, in_dt):
    u8, f32 = inputs(B, C, S)
    images = u8 if in_dt == U8 else f32
    partner = list(range(B - 1, -1, -1))  # the flip: the middle image is its own partner
    for box in box_sets(B, S):
        for lam in ([0.0, 0.37, 1.0, 0.37, 0.0][:B], [1.0] * B, [0.37] * B):
            out = call_mix(dev, torch.from_numpy(images), partner, lam, box, F32)
            compare_f32(out, images, partner, lam, box, f"in {in_dt} S {S} lam {lam[:3]} boxes {box[0]}..")
    box = boxes(B, S)
    # mixup alone: empty boxes everywhere
    out = call_mix(dev, torch.from_numpy(images), partner, [0.37] * B, [(0, 0, 0, 0)] * B, F32)
    compare_f32(out, images, partner, [0.37] * B, [(0, 0, 0, 0)] * B, f"in {in_dt} S {S} mixup")
    # one partner out of range on either side: that image mixes with itself
    bad = list(partner)
    bad[0], bad[-1] = B, -1
    out = call_mix(dev, torch.from_numpy(images), bad, [0.37] * B, box, F32)
    compare_f32(out, images, bad, [0.37] * B, box, f"in {in_dt} S {S} bad partner")
    n = R.normalize_u8_f32(images) if in_dt == U8 else images
    inside0 = R.inside_mask(box, S)[0]
    assert np.array_equal(out[0][:, inside0], n[0][:, inside0])  # its box holds its own pixels


@pytest.mark.parametrize("B,C,S", CASES)
def test_cutmix_u8_output_is_the_byte_select(dev, B, C, S):
    u8, _ = inputs(B, C, S)
    partner = list(range(B - 1, -1, -1))
    for box in box_sets(B, S):
        out = call_mix(dev, torch.from_numpy(u8), partner, None, box, U8)  # lam is not read: NULL
        ref = R.cutmix_u8_reference(u8, partner, box)
        print(f"S {S} boxes {box[0]}..: {int((out != ref).sum())} differing bytes of {ref.size}")
        assert np.array_equal(out, ref)
        # the normalised u8 result equals the fp32 route with lam = 1, bit for bit (what the engine reads either way)
        f = call_mix(dev, torch.from_numpy(u8), partner, [1.0] * B, box, F32)
        assert np.array_equal(R.normalize_u8_f32(out).view(np.uint32), f.view(np.uint32))
    box = boxes(B, S)
    bad = list(partner)
    bad[1] = 10 ** 6
    assert np.array_equal(call_mix(dev, torch.from_numpy(u8), bad, [0.5] * B, box, U8), R.cutmix_u8_reference(u8, bad, box))


def test_mix_u8_normalisation_is_the_engines(dev):
    """lam = 1, empty boxes: the output is normalize_u8 (evaluated on the host, as the other pixel tests do) of every byte value,
    bit for bit -- the contract of k_pixels.hip."""
    from ssrl_vit_mae_jepa_amd.data import normalize_u8
    x = torch.arange(256, dtype=torch.uint8).repeat(3).reshape(1, 3, 16, 16)
    out = call_mix(dev, x, [0], [1.0], [(0, 0, 0, 0)], F32)
    assert np.array_equal(out.view(np.uint32), normalize_u8(x).numpy().view(np.uint32))  # the host expression: IEEE division
    assert np.array_equal(out.view(np.uint32), R.normalize_u8_f32(x.numpy()).view(np.uint32))


def test_mix_rejections_before_launch(dev):
    from ssrl_vit_mae_jepa_amd._lib import lib
    u8, f32 = inputs(5, 3, 8)
    B = 5
    args = (list(range(B)), [0.5] * B, [(0, 4, 0, 4)] * B)
    sentinel = torch.full((B, 3, 8, 8), 201, dtype=torch.uint8, device=dev)
    assert call_mix(dev, torch.from_numpy(f32), *args, U8, out=sentinel, check_rc=False) != 0  # fp32 images -> uint8 output
    assert b"uint8" in lib.mae_last_error()
    torch.cuda.synchronize()
    assert bool((sentinel == 201).all())
    x = torch.from_numpy(f32).to(dev)
    assert call_mix(dev, x, *args, F32, out=x, check_rc=False) != 0  # in place
    assert b"overlap" in lib.mae_last_error()
    big = torch.zeros(2 * x.numel(), device=dev)
    half = x.numel() // 2
    big[:x.numel()].copy_(x.reshape(-1))
    src, dst = big[:x.numel()].view_as(x), big[half:half + x.numel()].view_as(x)  # a partial overlap
    assert call_mix(dev, src, *args, F32, out=dst, check_rc=False) != 0
    xu = torch.from_numpy(u8).to(dev)
    assert call_mix(dev, xu, *args, U8, out=xu, check_rc=False) != 0
    for bad_dt in (1, 3):  # bf16 images / an unknown dtype
        out = torch.empty(B, 3, 8, 8, device=dev)
        p, l, bx = (torch.zeros(B, dtype=torch.int32, device=dev), torch.ones(B, device=dev), torch.zeros(B, 4, dtype=torch.int32, device=dev))
        assert lib.mae_mix_batch(x.data_ptr(), bad_dt, p.data_ptr(), l.data_ptr(), bx.data_ptr(), B, 3, 8, F32, out.data_ptr(), stream(dev)) != 0
        assert lib.mae_mix_batch(x.data_ptr(), F32, p.data_ptr(), l.data_ptr(), bx.data_ptr(), B, 3, 8, bad_dt, out.data_ptr(), stream(dev)) != 0
    # a misaligned fp32 buffer at S % 4 == 0 (the 16-byte path) is refused; the same buffer at S = 7 (4-byte path) is not needed here
    odd = torch.zeros(x.numel() + 1, device=dev)[1:].view_as(x)
    assert call_mix(dev, odd, *args, F32, check_rc=False) != 0
    assert b"aligned" in lib.mae_last_error()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(f32))  # nothing was written


@pytest.mark.parametrize("B,S", [(5, 12), (3, 96)])
def test_mix_batch_wrapper(dev, B, S):
    """data.mix_batch: uint8 stays uint8 under pure CutMix, fp32 otherwise; yb = labels[partner]; the identity draw returns the batch."""
    from ssrl_vit_mae_jepa_amd.data import MixParams, draw_mix_params, mix_batch
    u8, _ = inputs(B, 3, S)
    x = torch.from_numpy(u8).to(dev)
    labels = torch.tensor([3, 1, 4, 1, 5][:B], device=dev)
    seen = set()
    for seed in range(12):
        p = draw_mix_params(B, S, seed, 0.8, 1.0, 1.0, 0.5)
        mixed, ya, yb, lam = mix_batch(x, labels, p)
        torch.cuda.synchronize()
        seen.add(p.cutmix)
        assert mixed.dtype == (torch.uint8 if p.cutmix else torch.float32)
        assert torch.equal(ya, labels) and torch.equal(yb, labels.flip(0)) and torch.equal(lam.cpu(), p.lam)
        if p.cutmix:
            assert np.array_equal(mixed.cpu().numpy(), R.cutmix_u8_reference(u8, p.partner.numpy(), p.box.numpy()))
        else:
            compare_f32(mixed.cpu().numpy(), u8, p.partner.numpy(), p.lam.numpy(), p.box.numpy(), f"wrapper seed {seed}")
    assert seen == {True, False}
    ident = draw_mix_params(B, S, 0, 0.8, 1.0, 0.0, 0.5)
    mixed, ya, yb, lam = mix_batch(x, labels, ident)
    assert mixed is x and torch.equal(yb, labels) and bool((lam == 1).all())
    # CutMix of an fp32 batch leaves as fp32; a draw that already lives on the device is taken as it is
    flip = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    cm = MixParams(flip, torch.full((B,), 0.75), torch.tensor([[0, 6, 0, 6]] * B, dtype=torch.int32), True)
    mixed, *_ = mix_batch(x.float(), labels, cm)
    assert mixed.dtype == torch.float32
    on_dev = MixParams(cm.partner.to(dev), cm.lam.to(dev), cm.box.to(dev), True)
    a, _ya, yb, _lam = mix_batch(x, labels, on_dev)
    b, *_ = mix_batch(x, labels, cm)
    assert a.dtype == torch.uint8 and torch.equal(a, b) and torch.equal(yb, labels.flip(0))
