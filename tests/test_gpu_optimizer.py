"""The optimizer step and the bf16 operand copies (k_loss_optim.hip through the C ABI) against tests/optim_ref.py, per element
(-m gpu).  Engines only: no model, no forward, no workspace; the tests fill the arenas themselves, with data generated on the
host over the whole trainable range (the 64-element padding between tensors included).

Every buffer handed to the library sits between guard elements filled with a bit pattern, the frozen tail of a parameter arena
carries the same pattern, and the weight cache is pre-filled with another: whatever a call must not write has to keep its bits.
Bounds are counted roundings (see optim_ref); bf16 copies are compared bit for bit."""
import functools
import math
import zlib

import numpy as np
import pytest
import torch

from ssrl_vit_mae_jepa_amd.mae import Engine
from tests import optim_ref as R
from tests.util import _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

GUARD = 256                 # elements in front of and behind every buffer
PAT32 = 0xDEADBEEF - (1 << 32)   # guard pattern of 4-byte buffers (as int32)
PAT16 = 0xBEEF - (1 << 16)       # guard pattern of 2-byte buffers (as int16)
FILL16 = 0x5A5A                  # what the weight cache holds before a call
INF = math.inf

CONFIGS = {
    "MICRO": dict(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2, decoder_embed_dim=64, decoder_depth=1,
                  decoder_num_heads=2),
    # matrices 4x96, 80x4, 240x80, 80x320: tile edges at 4, 16 and 64 + 16 in the 64x64 transpose tiles
    "EDGE": dict(image_size=8, patch_size=2, in_chans=1, embed_dim=80, depth=1, num_heads=5, decoder_embed_dim=96, decoder_depth=1,
                 decoder_num_heads=2),
    # 71 matrices: transpose_many needs two launches
    "DEEP": dict(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=15, num_heads=2, decoder_embed_dim=64, decoder_depth=2,
                 decoder_num_heads=2),
    # > 5.3M trainable elements: adamw_kernel wraps once, sumsq_kernel five times, the EMA boundary lies in adamw's second pass
    "WIDE": dict(image_size=32, patch_size=8, in_chans=3, embed_dim=192, depth=12, num_heads=3, decoder_embed_dim=64, decoder_depth=1,
                 decoder_num_heads=2),
}
PRECISIONS = ["fp32", "bf16"]
WORST = {}   # label -> (worst error / bound, case)


def note(label, ratio, case):
    if label not in WORST or ratio > WORST[label][0]:
        WORST[label] = (ratio, case)


@functools.lru_cache(maxsize=None)
def engine(name, precision) -> Engine:
    return Engine(CONFIGS[name], precision)


@functools.lru_cache(maxsize=None)
def layout(name):
    e = engine(name, "bf16")
    return R.wcache_layout(e.table, e.trainable_elems)


def offset_of(name, param):
    return next(off for n, off, _numel, _shape, _flags in engine(name, "fp32").table if n == param)


@functools.lru_cache(maxsize=6)
def case_for(name, hyper):
    """The shared inputs of one (config, hyperparameter set): generated once, never modified."""
    c = R.gen_case(engine(name, "fp32").trainable_elems, hyper, seed=zlib.crc32(f"{name}/{hyper}".encode()))
    for k in "pgmv":
        c[k].setflags(write=False)
    return c


class Buf:
    """n elements on the device between two guards of GUARD elements; ``fill`` (a bit pattern) or the guard pattern inside."""

    def __init__(self, n, dtype, dev, fill=None):
        self.n, self.dtype = n, dtype
        self.idt = torch.int32 if dtype == torch.float32 else torch.int16
        self.pat = PAT32 if dtype == torch.float32 else PAT16
        self.full = torch.full((GUARD + n + GUARD,), self.pat, dtype=self.idt, device=dev)
        self.bits = self.full[GUARD:GUARD + n]
        self.data = self.bits.view(dtype)
        if fill is not None:
            self.bits.fill_(fill)

    def load(self, arr, at=0):
        arr = np.ascontiguousarray(arr)
        t = torch.from_numpy(arr if arr.flags.writeable else arr.copy())   # the shared cases are read-only
        self.data[at:at + t.numel()].copy_(t)
        return self

    def host(self):
        """fp32 values, or the uint16 bit patterns of a bf16 buffer."""
        if self.dtype == torch.float32:
            return self.data.cpu().numpy()
        return self.bits.cpu().numpy().view(np.uint16)

    def guards_intact(self):
        return bool((self.full[:GUARD] == self.pat).all()) and bool((self.full[GUARD + self.n:] == self.pat).all())


class Arena:
    """Device state of one engine: params (arena_elems, the frozen tail left as pattern), grads / exp_avg / exp_avg_sq
    (trainable_elems), the weight cache (bf16 engines), stats and the reduction scratch."""

    def __init__(self, eng, dev):
        self.eng, self.T = eng, eng.trainable_elems
        self.p = Buf(eng.arena_elems, torch.float32, dev)
        self.g, self.m, self.v = (Buf(self.T, torch.float32, dev) for _ in range(3))
        self.w = Buf(eng.wcache_bytes // 2, torch.bfloat16, dev, FILL16) if eng.precision == "bf16" else None
        self.stats = Buf(2, torch.float32, dev)
        self.scratch = Buf(2048, torch.float32, dev)

    def load(self, c):
        for b, k in ((self.p, "p"), (self.g, "g"), (self.m, "m"), (self.v, "v")):
            b.load(c[k])
        if self.w is not None:
            self.w.bits.fill_(FILL16)
        return self

    def bufs(self):
        return [b for b in (self.p, self.g, self.m, self.v, self.w, self.stats, self.scratch) if b is not None]

    def assert_intact(self, what):
        torch.cuda.synchronize()
        for b in self.bufs():
            assert b.guards_intact(), f"{what}: a guard element was written"
        assert bool((self.p.bits[self.T:] == PAT32).all()), f"{what}: the frozen tail of the arena was written"

    def wptr(self):
        return _ptr(self.w.data) if self.w is not None else None

    def snapshot(self):
        return [b.full.clone() for b in (self.p, self.m, self.v, self.w) if b is not None]


def hyper_floats(c):
    return [float(c[k]) for k in ("lr", "b1", "b2", "eps", "wd")]


def adamw_range(ar, c, lo, count, dev):
    check(lib.mae_engine_adamw_range(ar.eng.handle, _ptr(ar.p.data), _ptr(ar.g.data), _ptr(ar.m.data), _ptr(ar.v.data), ar.wptr(),
                                     *hyper_floats(c), c["step"], _ptr(ar.stats.data), lo, count, stream(dev)))


def optimizer_step(ar, c, max_norm, dev, target=None, target_w=None, mom=None):
    common = [ar.eng.handle, _ptr(ar.p.data), _ptr(ar.g.data), _ptr(ar.m.data), _ptr(ar.v.data), ar.wptr(), *hyper_floats(c), float(max_norm),
              c["step"], _ptr(ar.stats.data), _ptr(ar.scratch.data)]
    if target is None:
        check(lib.mae_engine_optimizer_step(*common, stream(dev)))
    else:
        check(lib.mae_engine_optimizer_step_ema(*common, _ptr(target.data), _ptr(target_w.data) if target_w is not None else None, float(mom),
                                                stream(dev)))


def check_adamw(label, what, ar, c, coef=None):
    """p', m', v' inside the AdamW bounds; returns the fp32 p' the call wrote."""
    T = ar.T
    p_out, m_out, v_out = ar.p.host()[:T], ar.m.host(), ar.v.host()
    r = R.adamw_ratios(p_out, m_out, v_out, c, coef)
    print(f"{what}: error / bound  p' {r['p']:.3f}  m' {r['m']:.3f}  v' {r['v']:.3f}")
    for k in "pmv":
        note(f"{label} {k}'", r[k], what)
    assert max(r.values()) <= 1.0, (what, r)
    assert np.array_equal(ar.g.host(), c["g"]), f"{what}: the gradient was modified"
    return p_out


def expected_wcache(name, p_out, n_elems, straight=True, only=None):
    """The whole weight cache, bit for bit, after a refresh from the fp32 arena p_out: the straight copy, every transposed copy
    (``only``: a set of matrix names) and the pre-fill pattern everywhere else (the padding between transposed copies included)."""
    mats, trans = layout(name)
    T = p_out.size
    exp = np.full(n_elems, FILL16, dtype=np.uint16)
    if straight:
        exp[:T] = R.bf16_rne(p_out)
    for mt in mats:
        if only is None or mt["name"] in only:
            exp[mt["t_abs"]:mt["t_abs"] + mt["numel"]] = R.transposed_ref(p_out, mt)
    assert T + trans <= n_elems
    return exp


def assert_wcache(what, name, got, exp, T):
    if np.array_equal(got, exp):
        return
    bad = int(np.flatnonzero(got != exp)[0])
    where = "the straight copy"
    if bad >= T:
        where = "padding of the transposed region"
        for i, mt in enumerate(layout(name)[0]):
            if mt["t_abs"] <= bad < mt["t_abs"] + mt["numel"]:
                where = f"transposed matrix {i + 1} {mt['name']} ({mt['rows']}x{mt['cols']}), element {bad - mt['t_abs']}"
    raise AssertionError(f"{what}: weight cache element {bad} is {got[bad]:#06x}, expected {exp[bad]:#06x}: {where}")


# ------------------------------------------------------------------------------------------------ 1. AdamW per element
@pytest.mark.parametrize("n", [4, 1020, R.ADAMW_WRAP, R.ADAMW_WRAP + 4, 5_000_004])
def test_adamw_buffer_per_element(dev, n):
    eng = engine("MICRO", "fp32")
    c = R.gen_case(n, "step2", seed=n)
    bufs = {k: Buf(n, torch.float32, dev) for k in "pgmv"}
    stats = Buf(2, torch.float32, dev).load(np.array([c["norm"], c["coef"]], dtype=np.float32))
    runs = []
    for _ in range(2):
        for k in "pgmv":
            bufs[k].load(c[k])
        check(lib.mae_engine_adamw_buffer(eng.handle, *(_ptr(bufs[k].data) for k in "pgmv"), n, *hyper_floats(c), c["step"], _ptr(stats.data),
                                          stream(dev)))
        torch.cuda.synchronize()
        runs.append([bufs[k].bits.clone() for k in "pmv"])
    assert all(b.guards_intact() for b in bufs.values()) and stats.guards_intact(), f"n={n}: a guard element was written"
    assert all(torch.equal(a, b) for a, b in zip(*runs)), f"n={n}: the second run differs"
    assert np.array_equal(bufs["g"].host(), c["g"]) and np.array_equal(stats.host(), np.array([c["norm"], c["coef"]], dtype=np.float32))
    r = R.adamw_ratios(bufs["p"].host(), bufs["m"].host(), bufs["v"].host(), c)
    print(f"adamw_buffer n={n}: error / bound  p' {r['p']:.3f}  m' {r['m']:.3f}  v' {r['v']:.3f}")
    for k in "pmv":
        note(f"adamw_buffer {k}'", r[k], f"n={n}")
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("hyper", list(R.HYPER))
@pytest.mark.parametrize("name", list(CONFIGS))
def test_adamw_range_per_element(dev, name, hyper, precision):
    eng, c = engine(name, precision), case_for(name, hyper)
    ar, T, what = Arena(eng, dev), eng.trainable_elems, f"adamw_range {name} {hyper} {precision}"
    stats = np.array([c["norm"], c["coef"]], dtype=np.float32)
    runs = []
    for _ in range(2):
        ar.load(c).stats.load(stats)
        adamw_range(ar, c, 0, T, dev)
        ar.assert_intact(what)
        runs.append(ar.snapshot())
    assert all(torch.equal(a, b) for a, b in zip(*runs)), f"{what}: the second run differs"
    assert np.array_equal(ar.stats.host(), stats)
    p_out = check_adamw(f"adamw_range {precision}", what, ar, c)
    if precision == "bf16":
        # the straight copy is the rounded fp32 value the kernel wrote; adamw_range leaves the transposed region alone
        assert_wcache(what, name, ar.w.host(), expected_wcache(name, p_out, ar.w.n, only=set()), T)


# ------------------------------------------------------------------------------------------------ 2. shards
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["MICRO", "WIDE"])
def test_adamw_shards_equal_the_single_call(dev, name, precision):
    eng, c = engine(name, precision), case_for(name, "step2")
    ar, T, what = Arena(eng, dev), eng.trainable_elems, f"shards {name} {precision}"
    stats = np.array([c["norm"], c["coef"]], dtype=np.float32)
    ar.load(c).stats.load(stats)
    adamw_range(ar, c, 0, T, dev)
    ar.assert_intact(what)
    whole = ar.snapshot()
    a, b = T // 3 // 256 * 256 + 100, 2 * T // 3 // 256 * 256 + 36
    shards = [(a, b - a), (a, 0), (0, a), (b, T - b)]        # out of order, one empty; counts are multiples of 4, none of 256
    assert all(n % 4 == 0 and (n == 0 or n % 256) for _, n in shards) and sum(n for _, n in shards) == T
    ar.load(c).stats.load(stats)
    for lo, count in shards:
        before = ar.snapshot()
        adamw_range(ar, c, lo, count, dev)
        ar.assert_intact(f"{what} [{lo}, +{count})")
        for x, y in zip(before, ar.snapshot()):     # p, m, v (and the weight cache) share the element index
            assert torch.equal(x[:GUARD + lo], y[:GUARD + lo]) and torch.equal(x[GUARD + lo + count:], y[GUARD + lo + count:]), \
                f"{what}: the call on [{lo}, +{count}) wrote outside its shard"
            assert count == 0 or not torch.equal(x[GUARD + lo:GUARD + lo + count], y[GUARD + lo:GUARD + lo + count])
    assert all(torch.equal(x, y) for x, y in zip(whole, ar.snapshot())), f"{what}: the shards together differ from the single call"


# ------------------------------------------------------------------------------------------------ 3. sum of squares and clip
def _stats_check(label, what, stats, ref_sumsq, max_norm, k):
    norm, coef = R.clip(ref_sumsq, max_norm)
    quotient = R.f32(max_norm) / (norm + R.CLIP_EPS)
    rn = abs(float(stats[0]) - norm) / (R.norm_rel_bound(k) * norm) if norm else (0.0 if stats[0] == 0 else INF)
    rc = abs(float(stats[1]) - coef) / (R.coef_rel_bound(k) * quotient) if math.isfinite(quotient) else (0.0 if stats[1] == 1 else INF)
    print(f"{what}: norm {float(stats[0])!r} (fp64 {norm!r}) error / bound {rn:.3f}; coef {float(stats[1])!r} (fp64 {coef!r}) {rc:.3f}")
    note(f"{label} norm", rn, what)
    note(f"{label} coef", rc, what)
    assert rn <= 1.0 and rc <= 1.0, (what, rn, rc)


@pytest.mark.parametrize("n", [0, 4, 1020, R.SUMSQ_WRAP - 4, R.SUMSQ_WRAP, R.SUMSQ_WRAP + 4, R.ADAMW_WRAP + 4, 5_000_004])
def test_sumsq_buffer_and_clip(dev, n):
    eng = engine("MICRO", "fp32")
    g = R.gen_grad(max(n, 4), seed=n + 1)
    ref, k, prior = R.sumsq(g[:n]), R.sumsq_chain(n), 1234.5
    gbuf = Buf(g.size, torch.float32, dev).load(g)
    scratch = Buf(2048, torch.float32, dev)
    for accumulate in (0, 1):
        sums = Buf(2, torch.float32, dev).load(np.array([prior], dtype=np.float32))
        check(lib.mae_engine_grad_sumsq_buffer(eng.handle, _ptr(gbuf.data), n, accumulate, _ptr(sums.data), _ptr(scratch.data), stream(dev)))
        stats = Buf(2, torch.float32, dev)
        max_norm = R.f32(0.37 * math.sqrt(ref + accumulate * prior)) if n else 1.0
        check(lib.mae_engine_clip_from_sumsq(eng.handle, _ptr(sums.data), max_norm, _ptr(stats.data), stream(dev)))
        torch.cuda.synchronize()
        assert gbuf.guards_intact() and scratch.guards_intact() and sums.guards_intact() and stats.guards_intact()
        assert np.array_equal(gbuf.host(), g)
        out, what = sums.host(), f"sumsq_buffer n={n} accumulate={accumulate}"
        want = ref + accumulate * prior
        bound = R.sumsq_rel_bound(n) * ref + accumulate * R.SECOND * R.U * want
        ratio = abs(float(out[0]) - want) / bound if bound else (0.0 if float(out[0]) == want else INF)
        print(f"{what}: {float(out[0])!r} (fp64 {want!r}) error / bound {ratio:.3f}, chain {k}")
        note("sumsq", ratio, what)
        assert ratio <= 1.0, what
        if accumulate:
            assert abs(float(out[1]) - ref) <= R.sumsq_rel_bound(n) * ref, f"{what}: slot 1 holds the buffer's own sum"
        else:
            assert sums.bits[1].item() == PAT32, f"{what}: slot 1 was written"
        _stats_check("clip_from_sumsq", what, stats.host(), want, max_norm, k + accumulate)   # the sum with the prior total is one more rounding


@pytest.mark.parametrize("name,lo,short", [("MICRO", 0, 0), ("WIDE", 4 * 77, 4 * 13), ("WIDE", 0, 0)])
def test_sumsq_range(dev, name, lo, short):
    eng, c = engine(name, "fp32"), case_for(name, "step1")
    T = eng.trainable_elems
    count = T - lo - short
    gbuf, scratch = Buf(T, torch.float32, dev).load(c["g"]), Buf(2048, torch.float32, dev)
    for n in (count, 0):
        out = Buf(1, torch.float32, dev)
        check(lib.mae_engine_grad_sumsq_range(eng.handle, _ptr(gbuf.data), lo, n, _ptr(out.data), _ptr(scratch.data), stream(dev)))
        torch.cuda.synchronize()
        assert gbuf.guards_intact() and scratch.guards_intact() and out.guards_intact()
        ref, what = R.sumsq(c["g"][lo:lo + n]), f"sumsq_range {name} [{lo}, +{n})"
        got = float(out.host()[0])
        ratio = abs(got - ref) / (R.sumsq_rel_bound(n) * ref) if n else (0.0 if got == 0.0 else INF)
        print(f"{what}: {got!r} (fp64 {ref!r}) error / bound {ratio:.3f}")
        note("sumsq", ratio, what)
        assert ratio <= 1.0, what


@pytest.mark.parametrize("n", [R.SUMSQ_WRAP + 4, 5_000_004])
def test_sumsq_counts_every_float4_once(dev, n):
    """A gradient that is zero except +-2^j at probe positions: the sum of squares is an integer below 2^24, so every partial sum
    is exact in fp32 and the result must equal the fp64 sum bit for bit: a dropped or double-counted float4 cannot hide."""
    eng = engine("MICRO", "fp32")
    n4, wrap4 = n // 4, R.SUMSQ_WRAP // 4
    probes = [0, n4 - 1, 12345, min(700001, n4 - 2)]
    for w in range(1, -(-n4 // wrap4)):
        probes += [w * wrap4 - 1, w * wrap4]
    probes = sorted(set(probes))
    g = np.zeros(n, dtype=np.float32)
    for i, q in enumerate(probes):
        g[4 * q + i % 4] = (-1.0) ** i * 2.0 ** (i % 11)
    ref = R.sumsq(g)
    assert ref < 2 ** 24 and ref == sum(4.0 ** (i % 11) for i in range(len(probes)))
    gbuf, scratch, out = Buf(n, torch.float32, dev).load(g), Buf(2048, torch.float32, dev), Buf(1, torch.float32, dev)
    check(lib.mae_engine_grad_sumsq_buffer(eng.handle, _ptr(gbuf.data), n, 0, _ptr(out.data), _ptr(scratch.data), stream(dev)))
    torch.cuda.synchronize()
    assert gbuf.guards_intact() and scratch.guards_intact() and out.guards_intact()
    assert float(out.host()[0]) == ref, f"n={n}: {float(out.host()[0])!r} != {ref!r} with probes at float4 {probes}"
    for drop in (probes[-1], probes[len(probes) // 2]):      # one probe fewer: the sum drops by exactly that probe's square
        g2 = g.copy()
        g2[4 * drop:4 * drop + 4] = 0.0
        check(lib.mae_engine_grad_sumsq_buffer(eng.handle, _ptr(gbuf.load(g2).data), n, 0, _ptr(out.data), _ptr(scratch.data), stream(dev)))
        torch.cuda.synchronize()
        assert float(out.host()[0]) == R.sumsq(g2)


@pytest.mark.parametrize("total,max_norm,want", [(1e6, 1.0, None), (0.25, 1.0, 1.0), (1e6, INF, 1.0), (0.0, 1.0, 1.0), (0.0, INF, 1.0)],
                         ids=["active", "inactive", "inf", "zero", "zero_inf"])
def test_clip_cases(dev, total, max_norm, want):
    eng = engine("MICRO", "fp32")
    sums = Buf(2, torch.float32, dev).load(np.array([total], dtype=np.float32))
    stats = Buf(2, torch.float32, dev)
    check(lib.mae_engine_clip_from_sumsq(eng.handle, _ptr(sums.data), max_norm, _ptr(stats.data), stream(dev)))
    torch.cuda.synchronize()
    assert sums.guards_intact() and stats.guards_intact() and sums.bits[1].item() == PAT32 and float(sums.host()[0]) == total
    got = stats.host()
    norm, coef = R.clip(total, max_norm)
    assert float(got[0]) == norm, "the square roots of 1e6, 0.25 and 0 are exact"
    if want is not None:
        assert float(got[1]) == want == coef       # exactly 1: not clipped
    else:
        ratio = abs(float(got[1]) - coef) / (R.SECOND * 2 * R.U * coef)    # the sum with 1e-6f and the division
        note("clip_from_sumsq coef", ratio, "active, exact norm")
        assert coef < 1.0 and ratio <= 1.0


# ------------------------------------------------------------------------------------------------ 4. the fused step
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fused_step(dev, name, precision):
    eng, c = engine(name, precision), case_for(name, "step2")
    ar, T, what = Arena(eng, dev).load(c), eng.trainable_elems, f"optimizer_step {name} {precision}"
    max_norm = R.f32(0.37 * c["norm"])
    optimizer_step(ar, c, max_norm, dev)
    ar.assert_intact(what)
    stats = ar.stats.host()
    _stats_check("optimizer_step", what, stats, R.sumsq(c["g"]), max_norm, R.sumsq_chain(T))
    assert 0.3 < float(stats[1]) < 0.4
    p_out = check_adamw(f"optimizer_step {precision}", what, ar, c, coef=float(stats[1]))   # the coefficient the kernel read
    if precision == "fp32":
        return
    mats, _trans = layout(name)
    got, exp = ar.w.host(), expected_wcache(name, p_out, ar.w.n)
    if name == "DEEP":   # two launches of transpose_many: the 65th matrix opens the second one, the prediction head closes it
        assert len(mats) == 71 and mats[-1]["name"] == "decoder.decoder_pred.weight"
        for mt in (mats[64], mats[-1]):
            sl = slice(mt["t_abs"], mt["t_abs"] + mt["numel"])
            assert np.array_equal(got[sl], R.transposed_ref(p_out, mt)), f"{what}: transposed copy of {mt['name']}"
    assert_wcache(what, name, got, exp, T)


# ------------------------------------------------------------------------------------------------ 5. refresh of the copies
CRAFTED = np.array([
    0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000,     # ties: even upper half stays, odd upper half moves away from zero
    0x3F808001, 0x3F807FFF, 0x3F818001, 0x3F817FFF,     # just above / just below a tie
    0x00000000, 0x80000000,                             # +0, -0
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,     # the largest finite fp32 (rounds to infinity), the tie below it, the last that stays finite
    0x00800000, 0x80800000, 0x00800001, 0x00807FFF, 0x00808000,   # the smallest normals
], dtype=np.uint32).view(np.float32)


def crafted_arena(name):
    eng = engine(name, "bf16")
    mats, _ = layout(name)
    p = R.gen_params(eng.trainable_elems, seed=zlib.crc32(name.encode())).copy()
    k = CRAFTED.size
    p[:k] = CRAFTED
    for mt in mats:           # the first and the last elements of every matrix: a corner of its first and of its last tile
        p[mt["offset"]:mt["offset"] + k] = CRAFTED
        p[mt["offset"] + mt["numel"] - k:mt["offset"] + mt["numel"]] = CRAFTED
    return p


@pytest.mark.parametrize("name", ["MICRO", "EDGE", "DEEP"])
def test_refresh_weights_bit_exact(dev, name):
    eng = engine(name, "bf16")
    ar, T, what = Arena(eng, dev), eng.trainable_elems, f"refresh_weights {name}"
    p = crafted_arena(name)
    ar.p.load(p)
    check(lib.mae_engine_refresh_weights(eng.handle, _ptr(ar.p.data), _ptr(ar.w.data), stream(dev)))
    ar.assert_intact(what)
    assert np.array_equal(ar.p.host()[:T].view(np.uint32), p.view(np.uint32)), f"{what}: the parameters were modified"
    assert_wcache(what, name, ar.w.host(), expected_wcache(name, p, ar.w.n), T)

    # a range that cuts through a matrix at each end: only the matrices that lie inside it are rewritten
    mats, _ = layout(name)
    first, last = mats[1], mats[-2]
    lo, hi = first["offset"] + 8, last["offset"] + last["numel"] - 8
    inside = {mt["name"] for mt in mats if mt["offset"] >= lo and mt["offset"] + mt["numel"] <= hi}
    assert inside == {mt["name"] for mt in mats[2:-2]} and (name != "DEEP" or len(inside) > 64)
    ar.w.bits.fill_(FILL16)
    check(lib.mae_engine_refresh_transposed_range(eng.handle, _ptr(ar.p.data), _ptr(ar.w.data), lo, hi - lo, stream(dev)))
    ar.assert_intact(what + " range")
    assert_wcache(what + " range", name, ar.w.host(), expected_wcache(name, p, ar.w.n, straight=False, only=inside), T)
    # exactly one matrix, then nothing
    one = mats[len(mats) // 2]
    ar.w.bits.fill_(FILL16)
    check(lib.mae_engine_refresh_transposed_range(eng.handle, _ptr(ar.p.data), _ptr(ar.w.data), one["offset"], one["numel"], stream(dev)))
    ar.assert_intact(what + " one matrix")
    assert_wcache(what + " one matrix", name, ar.w.host(), expected_wcache(name, p, ar.w.n, straight=False, only={one["name"]}), T)
    ar.w.bits.fill_(FILL16)
    check(lib.mae_engine_refresh_transposed_range(eng.handle, _ptr(ar.p.data), _ptr(ar.w.data), one["offset"], 0, stream(dev)))
    check(lib.mae_engine_refresh_transposed_range(eng.handle, _ptr(ar.p.data), _ptr(ar.w.data), one["offset"] + 1, one["numel"] - 1, stream(dev)))
    ar.assert_intact(what + " empty")
    assert bool((ar.w.bits == FILL16).all()), f"{what}: count = 0 or a range holding no whole matrix wrote the weight cache"


def test_refresh_weights_fp32_engine_writes_nothing(dev):
    eng = engine("MICRO", "fp32")
    ar = Arena(eng, dev)
    ar.p.load(crafted_arena("MICRO"))
    w = Buf(1024, torch.bfloat16, dev, FILL16)
    check(lib.mae_engine_refresh_weights(eng.handle, _ptr(ar.p.data), _ptr(w.data), stream(dev)))
    check(lib.mae_engine_refresh_transposed_range(eng.handle, _ptr(ar.p.data), _ptr(w.data), 0, eng.trainable_elems, stream(dev)))
    ar.assert_intact("fp32 refresh")
    assert w.guards_intact() and bool((w.bits == FILL16).all())


# ------------------------------------------------------------------------------------------------ 6. EMA
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["MICRO", "WIDE"])
def test_ema_step(dev, name, precision):
    eng, c = engine(name, precision), case_for(name, "step2")
    ar, T, what = Arena(eng, dev).load(c), eng.trainable_elems, f"optimizer_step_ema {name} {precision}"
    ema_n = offset_of(name, "decoder.mask_token")
    assert 0 < ema_n < T and ema_n % 4 == 0 and (name != "WIDE" or R.ADAMW_WRAP < ema_n < T - 4)
    optimizer_step(ar, c, INF, dev)
    ar.assert_intact(what)
    plain, plain_stats = ar.snapshot(), ar.stats.host().copy()
    assert float(plain_stats[1]) == 1.0
    p_out = check_adamw(f"optimizer_step {precision}", what + " (plain step, coef 1)", ar, c, coef=1.0)
    t0 = R.gen_params(T, seed=zlib.crc32(f"{name}/target".encode()))
    tgt = Buf(eng.arena_elems, torch.float32, dev)
    tgt_w = Buf(eng.wcache_bytes // 2, torch.bfloat16, dev) if precision == "bf16" else None
    for mom in (0.996, 0.3, 0.0, 1.0):
        ar.load(c)
        tgt.load(t0)
        if tgt_w is not None:
            tgt_w.bits.fill_(FILL16)
        optimizer_step(ar, c, INF, dev, tgt, tgt_w, mom)
        ar.assert_intact(f"{what} mom={mom}")
        assert tgt.guards_intact() and (tgt_w is None or tgt_w.guards_intact())
        assert all(torch.equal(x, y) for x, y in zip(plain, ar.snapshot())) and np.array_equal(ar.stats.host(), plain_stats), \
            f"{what} mom={mom}: the step itself differs from mae_engine_optimizer_step"
        t_all = tgt.data.cpu().numpy()
        t_out = t_all[:ema_n]
        assert np.array_equal(t_all[ema_n:T].view(np.uint32), t0[ema_n:].view(np.uint32)), f"{what} mom={mom}: the target past the encoder was written"
        assert bool((tgt.bits[T:] == PAT32).all()), f"{what} mom={mom}: the target's frozen tail was written"
        if mom == 1.0:
            assert np.array_equal(t_out.view(np.uint32), t0[:ema_n].view(np.uint32)), f"{what}: momentum 1 must leave the target unchanged"
        elif mom == 0.0:
            assert np.array_equal(t_out.view(np.uint32), p_out[:ema_n].view(np.uint32)), f"{what}: momentum 0 must copy the parameters"
        ratio = R.worst_ratio(t_out, R.ema(t0[:ema_n], p_out[:ema_n], mom), R.ema_bound(t0[:ema_n], p_out[:ema_n], mom))
        print(f"{what} mom={mom}: error / bound {ratio:.3f}")
        note(f"ema {precision}", ratio, f"{name} mom={mom}")
        assert ratio <= 1.0, (what, mom, ratio)
        if tgt_w is not None:
            exp = np.full(tgt_w.n, FILL16, dtype=np.uint16)
            exp[:ema_n] = R.bf16_rne(t_out)
            got = tgt_w.host()
            assert np.array_equal(got[:ema_n], exp[:ema_n]), f"{what} mom={mom}: the target's bf16 copy is not the rounded target"
            assert np.array_equal(got[ema_n:], exp[ema_n:]), f"{what} mom={mom}: the target's weight cache past the encoder was written"


# ------------------------------------------------------------------------------------------------ 7. argument checks
@pytest.mark.parametrize("precision", PRECISIONS)
def test_bad_arguments_are_refused_before_any_launch(dev, precision):
    eng, c = engine("MICRO", precision), case_for("MICRO", "step2")
    ar, T, h = Arena(eng, dev).load(c), eng.trainable_elems, eng.handle
    ar.stats.load(np.array([c["norm"], c["coef"]], dtype=np.float32))
    tgt = Buf(eng.arena_elems, torch.float32, dev).load(c["p"])
    tgt_w = Buf(eng.wcache_bytes // 2, torch.bfloat16, dev, FILL16)
    sums = Buf(2, torch.float32, dev)
    torch.cuda.synchronize()
    everything = ar.bufs() + [tgt, tgt_w, sums]
    before = [b.full.clone() for b in everything]
    P, G, M, V, W, S, X = (_ptr(ar.p.data), _ptr(ar.g.data), _ptr(ar.m.data), _ptr(ar.v.data), ar.wptr(), _ptr(ar.stats.data), _ptr(ar.scratch.data))
    hy, st, s = hyper_floats(c), c["step"], stream(dev)
    bad = {
        "adamw_range lo % 4": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, W, *hy, st, S, 2, 64, s),
        "adamw_range count % 4": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, W, *hy, st, S, 0, 62, s),
        "adamw_range past the end": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, W, *hy, st, S, T - 4, 8, s),
        "adamw_range negative lo": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, W, *hy, st, S, -4, 8, s),
        "adamw_range step 0": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, W, *hy, 0, S, 0, T, s),
        "adamw_buffer count % 4": lambda: lib.mae_engine_adamw_buffer(h, P, G, M, V, 62, *hy, st, S, s),
        "adamw_buffer step 0": lambda: lib.mae_engine_adamw_buffer(h, P, G, M, V, 64, *hy, 0, S, s),
        "sumsq_range lo % 4": lambda: lib.mae_engine_grad_sumsq_range(h, G, 2, 64, _ptr(sums.data), X, s),
        "sumsq_range count % 4": lambda: lib.mae_engine_grad_sumsq_range(h, G, 0, 62, _ptr(sums.data), X, s),
        "sumsq_range past the end": lambda: lib.mae_engine_grad_sumsq_range(h, G, T - 4, 8, _ptr(sums.data), X, s),
        "sumsq_buffer count % 4": lambda: lib.mae_engine_grad_sumsq_buffer(h, G, 62, 0, _ptr(sums.data), X, s),
        "refresh_transposed_range past the end": lambda: lib.mae_engine_refresh_transposed_range(h, P, W, T - 4, 8, s),
        "optimizer_step step 0": lambda: lib.mae_engine_optimizer_step(h, P, G, M, V, W, *hy, 1.0, 0, S, X, s),
        "ema momentum > 1": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, st, S, X, _ptr(tgt.data), _ptr(tgt_w.data), 1.5, s),
        "ema momentum < 0": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, st, S, X, _ptr(tgt.data), _ptr(tgt_w.data), -0.01, s),
        "ema momentum nan": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, st, S, X, _ptr(tgt.data), _ptr(tgt_w.data), math.nan, s),
        "ema null target": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, st, S, X, None, _ptr(tgt_w.data), 0.5, s),
        "ema step 0": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, 0, S, X, _ptr(tgt.data), _ptr(tgt_w.data), 0.5, s),
    }
    if precision == "bf16":
        bad.update({
            "optimizer_step null wcache": lambda: lib.mae_engine_optimizer_step(h, P, G, M, V, None, *hy, 1.0, st, S, X, s),
            "adamw_range null wcache": lambda: lib.mae_engine_adamw_range(h, P, G, M, V, None, *hy, st, S, 0, T, s),
            "refresh_weights null wcache": lambda: lib.mae_engine_refresh_weights(h, P, None, s),
            "refresh_transposed_range null wcache": lambda: lib.mae_engine_refresh_transposed_range(h, P, None, 0, T, s),
            "ema null target wcache": lambda: lib.mae_engine_optimizer_step_ema(h, P, G, M, V, W, *hy, 1.0, st, S, X, _ptr(tgt.data), None, 0.5, s),
        })
    for what, call in bad.items():
        rc = call()
        msg = lib.mae_last_error()
        assert rc != 0 and msg and len(msg) > 8, f"{what}: accepted (rc {rc}, message {msg!r})"
        torch.cuda.synchronize()
        for b, x in zip(everything, before):
            assert torch.equal(b.full, x), f"{what}: refused, but something was written"
    check(0)     # releases the tensors the pointers above kept alive


def test_zz_report():
    """Prints the worst error / bound seen per quantity: a record of how much of each counted bound the kernels use."""
    print("\nworst error / bound per quantity:")
    for label, (ratio, case) in sorted(WORST.items()):
        print(f"  {label:28s} {ratio:.3f}  ({case})")
