"""mae_engine_grad_accumulate (k_loss_optim.hip through the C ABI) per element (-m gpu): dst = (overwrite ? 0 : dst) + src over
[lo, lo + count).  One IEEE fp32 add per element, so the result must equal numpy's fp32 sum bit for bit (NaNs compared as values)
and the source bit for bit under overwrite: the bound is zero.  Plain buffers between guards, as tests/test_gpu_optimizer.py:
the guards keep their pattern and everything outside the range keeps its bits; refused calls leave every bit alone."""
import functools

import numpy as np
import pytest
import torch

from ssrl_vit_mae_jepa_amd import _lib
from ssrl_vit_mae_jepa_amd.mae import Engine
from tests import accum_ref as R
from tests.util import _ptr, lib, stream

pytestmark = pytest.mark.gpu

GUARD = 256
PAT32 = 0xDEADBEEF - (1 << 32)
SWEEP = _lib.GRAD_ACC_BLOCKS * 1024   # floats one pass of the capped grid covers: blocks x 256 threads x 4 floats
COUNTS = [0, 4, 252, 1024, 1028, SWEEP - 4, SWEEP, SWEEP + 4, 2 * SWEEP + 8]
LOS = [0, 4, 64, 4096 + 64]
MICRO = dict(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


@functools.lru_cache(maxsize=None)
def engine() -> Engine:
    return Engine(MICRO, "fp32")


class Buf:
    """n floats on the device between two guards of GUARD elements filled with a bit pattern."""

    def __init__(self, arr, dev):
        self.n = arr.size
        self.full = torch.full((GUARD + self.n + GUARD,), PAT32, dtype=torch.int32, device=dev)
        self.data = self.full[GUARD:GUARD + self.n].view(torch.float32)
        self.data.copy_(torch.from_numpy(np.array(arr)))
        self.before = self.full.clone()

    def host(self):
        return self.data.cpu().numpy()

    def guards_intact(self):
        return bool((self.full[:GUARD] == PAT32).all()) and bool((self.full[GUARD + self.n:] == PAT32).all())

    def unchanged(self):
        return bool(torch.equal(self.full, self.before))


def accumulate(dst, src, lo, count, overwrite, dev):
    return lib.mae_engine_grad_accumulate(engine().handle, _ptr(dst), _ptr(src), lo, count, int(overwrite), stream(dev))


@functools.lru_cache(maxsize=None)
def inputs(n):
    d, s = R.accumulate_inputs(n, seed=n % 9973)
    d.setflags(write=False), s.setflags(write=False)
    return d, s


@pytest.mark.parametrize("overwrite", [False, True])
@pytest.mark.parametrize("count", COUNTS)
def test_range_is_one_fp32_add_per_element(dev, count, overwrite):
    for lo in (LOS if count <= 1028 else LOS[:2] if count < 2 * SWEEP else LOS[1:2]):
        n = lo + count + 68                                 # 68 floats behind the range stay as they are
        d0, s0 = inputs(n)
        dst, src = Buf(d0, dev), Buf(s0, dev)
        assert accumulate(dst.data, src.data, lo, count, overwrite, dev) == 0, lib.mae_last_error()
        torch.cuda.synchronize()
        out = dst.host()
        want = s0[lo:lo + count] if overwrite else R.add_f32(d0[lo:lo + count], s0[lo:lo + count])
        what = f"count {count} lo {lo} overwrite {overwrite}"
        if overwrite:
            assert np.array_equal(out[lo:lo + count].view(np.uint32), want.view(np.uint32)), what      # the source's bits, NaN payloads included
        else:
            assert R.same_values(out[lo:lo + count], want), what
        assert np.array_equal(out[:lo].view(np.uint32), d0[:lo].view(np.uint32)), what + ": written in front of the range"
        assert np.array_equal(out[lo + count:].view(np.uint32), d0[lo + count:].view(np.uint32)), what + ": written behind the range"
        assert dst.guards_intact() and src.unchanged(), what


def test_two_calls_are_two_adds(dev):
    n = 4096 + 252
    d0, s0 = inputs(n)
    s1 = np.roll(s0, 17)
    dst, a, b = Buf(d0, dev), Buf(s0, dev), Buf(s1, dev)
    assert accumulate(dst.data, a.data, 0, n, False, dev) == 0 and accumulate(dst.data, b.data, 0, n, False, dev) == 0
    torch.cuda.synchronize()
    assert R.same_values(dst.host(), R.add_f32(R.add_f32(d0, s0), s1))
    # a window as the modules run it: overwrite, accumulate, then the stash added into a live buffer
    stash, live = Buf(d0, dev), Buf(s1, dev)
    assert accumulate(stash.data, a.data, 0, n, True, dev) == 0 and accumulate(stash.data, b.data, 0, n, False, dev) == 0
    assert accumulate(live.data, stash.data, 0, n, False, dev) == 0
    torch.cuda.synchronize()
    assert R.same_values(live.host(), R.add_f32(s1, R.add_f32(s0, s1)))
    assert dst.guards_intact() and stash.guards_intact() and live.guards_intact() and a.unchanged() and b.unchanged()


def test_rejections_touch_nothing(dev):
    n = 1024
    d0, s0 = inputs(n)
    dst, src = Buf(d0, dev), Buf(s0, dev)
    h, s = engine().handle, stream(dev)
    D, S = dst.data, src.data
    cases = {
        "odd lo": lambda: accumulate(D, S, 2, 64, False, dev),
        "odd count": lambda: accumulate(D, S, 0, 62, False, dev),
        "negative lo": lambda: accumulate(D, S, -4, 64, False, dev),
        "negative count": lambda: accumulate(D, S, 0, -4, False, dev),
        "misaligned dst": lambda: accumulate(D[1:], S, 0, 64, False, dev),
        "misaligned src": lambda: accumulate(D, S[2:], 0, 64, True, dev),
        "misaligned both, count 0": lambda: accumulate(D[1:], S[1:], 0, 0, False, dev),
        "null dst": lambda: lib.mae_engine_grad_accumulate(h, None, _ptr(S), 0, 64, 0, s),
        "null src": lambda: lib.mae_engine_grad_accumulate(h, _ptr(D), None, 0, 64, 0, s),
        "null engine": lambda: lib.mae_engine_grad_accumulate(None, _ptr(D), _ptr(S), 0, 64, 0, s),
        "same buffer": lambda: accumulate(D, D, 0, 64, False, dev),
        "overlap from behind": lambda: accumulate(D, D[32:], 0, 64, False, dev),
        "overlap from the front": lambda: accumulate(D[32:], D, 0, 64, True, dev),
        "overlap by one vector": lambda: accumulate(D, D[60:], 0, 64, False, dev),
    }
    for what, call in cases.items():
        rc = call()
        _lib.check(0)   # releases the tensors ptr() kept for the call
        assert rc != 0, what
        msg = lib.mae_last_error()
        assert msg and b"mae_engine_grad_accumulate" in msg, (what, msg)
    torch.cuda.synchronize()
    assert dst.unchanged() and src.unchanged()
    # touching ranges do not overlap; count 0 is a successful no-op without a launch, whatever the buffers hold
    assert accumulate(D, D[64:], 0, 64, False, dev) == 0
    torch.cuda.synchronize()
    out = dst.host()
    assert R.same_values(out[:64], R.add_f32(d0[:64], d0[64:128])) and np.array_equal(out[64:].view(np.uint32), d0[64:].view(np.uint32))
    before = dst.full.clone()
    assert accumulate(D, S, 64, 0, False, dev) == 0 and accumulate(D, D, 0, 0, True, dev) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst.full, before) and src.unchanged()
