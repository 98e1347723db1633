"""mae_classifier_head_soft on the MI355X against the fp64 soft-target reference of tests/mix_ref.py: both head kernels (the
class-token / all-row head and the row-range head), both dtypes, label smoothing on and off, per-row lam including 0 and 1;
a bad second label, bit-equal repeats, and the hard-label call bit for bit when nothing soft is asked for."""
import math

import pytest
import torch

import tests.test_gpu_patch_classifier as TP
from tests import mix_ref as R
from tests.util import BF16, F32, TDT, rel_err, stream

pytestmark = pytest.mark.gpu

# (with_cls, pool of the C ABI, reference pool, first pooled row): cls and mean run classifier_head_kernel, the patch-row means
# (with and without a class token) classifier_head_range_kernel
POOLS = {"cls": (1, 0, "cls", 0), "mean": (1, 1, "mean", 0), "patches_with_cls": (1, 2, "mean", 1), "patch_only": (0, 1, "mean", 0)}
SHAPES = [(1, 2, 144), (7, 10, 384), (7, 100, 1024)]
ROWS = 6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def run_soft(dev, feats, dt, with_cls, pool, head, C, ya, yb, lam, eps, grad_scale=1.0, check_rc=True):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    B, rows, D = feats.shape
    f = feats.to(dev, TDT[dt]).contiguous()
    h = head.to(dev).contiguous()
    la = ya.to(dev).contiguous()
    lb = yb.to(dev).contiguous() if yb is not None else None
    lm = lam.to(dev, torch.float32).contiguous() if lam is not None else None
    logits = torch.empty(B, C, device=dev)
    loss = torch.empty(1, device=dev)
    correct = torch.empty(1, dtype=torch.int32, device=dev)
    hg = torch.full((C * D + C,), float("nan"), device=dev)
    dfeat = torch.full((B, D) if pool == 0 else (B, rows, D), float("nan"), dtype=TDT[dt], device=dev)
    n = lib.mae_classifier_head_scratch_bytes(B, C, D)
    scratch = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib.mae_classifier_head_soft(_ptr(f), dt, B, rows, D, with_cls, pool, _ptr(h), C, _ptr(la), float(grad_scale), _ptr(logits), _ptr(loss),
                                      _ptr(correct), _ptr(hg), _ptr(dfeat), _ptr(scratch), n, _ptr(lb), _ptr(lm), float(eps), stream(dev))
    if not check_rc:
        check(0)
        return rc
    check(rc)
    torch.cuda.synchronize()
    return logits.cpu(), loss.cpu()[0], int(correct.cpu()[0]), hg.cpu(), dfeat.float().cpu()


_inputs = {}


def inputs(B, C, D):
    if (B, C, D) not in _inputs:
        g = torch.Generator().manual_seed(B * 131 + C * 7 + D)
        feats = torch.randn(B, ROWS, D, generator=g)
        head = torch.cat([torch.randn(C * D, generator=g) * D ** -0.5, torch.randn(C, generator=g) * 0.1])
        ya, yb = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
        lam = torch.rand(B, generator=g)
        lam[0] = 0.0 if B > 1 else 0.37
        if B > 2:
            lam[1], yb[2] = 1.0, ya[2]
        _inputs[(B, C, D)] = (feats, head, ya, yb, lam, {})
    return _inputs[(B, C, D)]


@pytest.mark.parametrize("B,C,D", SHAPES)
@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_soft_head_matches_fp64(dev, B, C, D, pool, eps, dt):
    feats, head, ya, yb, lam, refs = inputs(B, C, D)
    with_cls, abi_pool, ref_pool, lo = POOLS[pool]
    bf = dt == BF16
    key = (ref_pool, lo, eps, bf)
    if key not in refs:
        refs[key] = R.soft_head_reference(feats, ref_pool, lo, head, C, ya, yb, lam, eps, bf, grad_scale=0.5)
    lr, lossr, correctr, hgr, dfr = refs[key]
    logits, loss, correct, hg, dfeat = run_soft(dev, feats, dt, with_cls, abi_pool, head, C, ya, yb, lam, eps, grad_scale=0.5)
    tol = 2e-3 if bf else 1e-5
    print(f"logits {rel_err(logits, lr):.3e} loss {abs(float(loss) - float(lossr)):.3e} head_grads {rel_err(hg, hgr):.3e} d_feats {rel_err(dfeat, dfr):.3e}")
    assert rel_err(logits, lr) < tol
    assert abs(float(loss) - float(lossr)) <= tol * max(1.0, abs(float(lossr)))
    assert correct == int((logits.argmax(1) == ya).sum())  # against ya, exact on the engine's own logits
    if not bf:
        assert correct == correctr
    assert rel_err(hg, hgr) < (2e-2 if bf else 1e-4)
    assert rel_err(dfeat, dfr) < (2e-2 if bf else 1e-4)
    assert torch.isfinite(dfeat).all()
    again = run_soft(dev, feats, dt, with_cls, abi_pool, head, C, ya, yb, lam, eps, grad_scale=0.5)
    for x, y in zip((logits, loss, correct, hg, dfeat), again):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))  # two runs, the same bits


@pytest.mark.parametrize("pool", ["cls", "patch_only"])
def test_soft_defaults_mean_what_the_header_says(dev, pool):
    """labels_b NULL = labels and lam NULL = 1: smoothing alone equals the explicit pair (ya, ya, 1) bit for bit."""
    feats, head, ya, _yb, _lam, _ = inputs(7, 10, 384)
    with_cls, abi_pool, _rp, _lo = POOLS[pool]
    a = run_soft(dev, feats, BF16, with_cls, abi_pool, head, 10, ya, None, None, 0.1)
    b = run_soft(dev, feats, BF16, with_cls, abi_pool, head, 10, ya, ya, torch.ones(7), 0.1)
    for x, y in zip(a, b):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


@pytest.mark.parametrize("pool", ["mean", "patches_with_cls"])
def test_bad_second_label_gives_a_nan_row(dev, pool):
    feats, head, ya, yb, lam, _ = inputs(7, 10, 384)
    with_cls, abi_pool, ref_pool, lo = POOLS[pool]
    for bad_value in (10, -1, 2 ** 40):
        bad = yb.clone()
        bad[3] = bad_value
        logits, loss, correct, hg, dfeat = run_soft(dev, feats, F32, with_cls, abi_pool, head, 10, ya, bad, lam, 0.1)
        assert math.isnan(float(loss))
        assert correct == int((logits.argmax(1) == ya).sum())  # ya is fine in every row
        assert torch.isnan(dfeat[3, lo:]).all() and torch.isfinite(dfeat[:3]).all() and torch.isfinite(dfeat[4:]).all()
    # the other rows are what they are without the bad row's neighbours: compare with the reference on the good rows
    good = [0, 1, 2, 4, 5, 6]
    ref = R.soft_head_reference(feats, ref_pool, lo, head, 10, ya, yb, lam, 0.1, False)
    assert rel_err(dfeat[good], ref[4][good]) < 1e-4
    # a bad first label: NaN too, and not counted as correct
    bad_a = ya.clone()
    bad_a[0] = 10
    logits, loss, correct, _hg, dfeat = run_soft(dev, feats, F32, with_cls, abi_pool, head, 10, bad_a, yb, lam, 0.1)
    assert math.isnan(float(loss)) and torch.isnan(dfeat[0, lo:]).all()
    assert correct == int((logits.argmax(1)[1:] == ya[1:]).sum())


@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("dt", [F32, BF16])
def test_nothing_soft_is_the_hard_call_bit_for_bit(dev, pool, dt):
    feats, head, ya, _yb, _lam, _ = inputs(7, 10, 384)
    with_cls, abi_pool, _rp, _lo = POOLS[pool]
    soft = run_soft(dev, feats, dt, with_cls, abi_pool, head, 10, ya, None, None, 0.0, grad_scale=0.5)
    hard = TP.run_head_ex(dev, feats, dt, with_cls, abi_pool, head, 10, ya, grad_scale=0.5)
    for i, (x, y) in enumerate(zip(soft, hard)):
        x, y = torch.as_tensor(x), torch.as_tensor(y)
        if pool == "cls" and i == 4:  # the hard runner's d_feats buffer is (B, rows, D): the class rows' gradient fills its first B * D
            y = y.reshape(-1)[:x.numel()].view_as(x)
        assert torch.equal(x, y), i
    # the soft kernel at lam = 1, ya == yb, eps = 0 computes the same loss to rounding (another instantiation, not the same bits)
    one = run_soft(dev, feats, dt, with_cls, abi_pool, head, 10, ya, ya, torch.ones(7), 0.0, grad_scale=0.5)
    assert abs(float(one[1]) - float(soft[1])) <= 1e-6 * abs(float(soft[1])) and rel_err(one[3], soft[3]) < 1e-5


def test_soft_rejections(dev):
    from ssrl_vit_mae_jepa_amd._lib import lib
    feats, head, ya, yb, lam, _ = inputs(7, 10, 384)
    for eps in (1.0, -0.1, float("nan")):
        assert run_soft(dev, feats, F32, 1, 0, head, 10, ya, yb, lam, eps, check_rc=False) != 0
        assert b"label_smoothing" in lib.mae_last_error()
    assert run_soft(dev, feats, F32, 0, 0, head, 10, ya, yb, lam, 0.1, check_rc=False) != 0  # cls pool without a class token
