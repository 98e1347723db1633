"""mae_attention_fwd / mae_attention_bwd through the C ABI against tests/attn_ref.py, element by element (-m gpu).

Every case of attn_ref.cases(): the smallest length of every route the dispatch can select for hd in {16, 24, 32, 48, 64}, T <= 1024 and
both dtypes (both sides of every LDS threshold), the lengths inside each chunk class, the remainders of the XCD remap, operands 8 bytes
off a 16-byte boundary, one and three heads of 24.  One test runs forward and backward of a case on four inputs: normal values at
sigma = 1 and 3 inside the per-element bound; key routing (out = V[sigma] and, in bf16, dV = dO[sigma^-1] bit for bit, lse, dQ, dK
inside the bound); key counting (out = count / T to 2 fp32 ulps, lse = log T).  The backward is given the reference's lse and out, so it
is judged alone.  Every output lives in a buffer of payload NaNs with guards on both sides; three launches go out back to back and must
agree bit for bit, no guard may change, no output element may keep the fill value.  test_zz_report prints the label table and the
worst error / bound per label and output.

The whole file (188 tests) takes about 9 s on an MI355X; the largest case (fp32, T = 961, hd = 64) 0.25 s.  The repeat check found
the missing barrier in front of zero_pad_chunks (bf16-B1-T257-H2-hd24: the second backward launch differed from the first)."""
import pytest
import torch

from tests import attn_ref as R
from tests.util import BF16, F32, _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in R.cases()}
DT = {"bf16": (BF16, torch.bfloat16), "f32": (F32, torch.float32)}
WORST = {}   # (direction label, output) -> (worst error / bound, case id, family)
EXACT = {"checked": 0, "differing": 0}


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def _bits(x):
    return x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32)


def _place(x, dev, off):
    """x on the device, `off` elements past an aligned address."""
    buf = torch.empty(x.numel() + off, dtype=x.dtype, device=dev)
    v = buf[off:].view(x.shape)
    v.copy_(x)
    assert v.data_ptr() % 16 == (off * x.element_size()) % 16
    return v


def _launch3(what, dev, shapes, call, off):
    """Three back-to-back launches into three sets of guarded fill-valued buffers -> the first set's views.  All sets must agree bit
    for bit (guards included, so the NaN fill compares as bits), no guard may change."""
    sets = []
    for _ in range(3):
        bufs = [R.guarded(shape, dtype, dev, off if o else 0) for shape, dtype, o in shapes]
        sets.append(bufs)
    for bufs in sets:
        call(*[v for _, v in bufs])
    torch.cuda.synchronize()
    for n, bufs in enumerate(sets[1:], 2):
        for (b0, _), (b, _) in zip(sets[0], bufs):
            assert torch.equal(_bits(b0), _bits(b)), f"{what}: launch {n} differs from launch 1"
    for (buf, view), (shape, dtype, o) in zip(sets[0], shapes):
        assert R.guards_touched(buf, view, off if o else 0) == 0, f"{what}: a guard element changed"
    return [v for _, v in sets[0]]


def _run(c, dev, qkv, do, r, what):
    """Forward on qkv, backward on (qkv, reference out, do, reference lse) -> out, lse, d_qkv."""
    dt, tdt = DT[c.dtype]
    off = (8 // torch.empty(0, dtype=tdt).element_size()) if c.offset8 else 0
    s = stream(dev)
    q, g = _place(qkv, dev, off), _place(do, dev, off)
    o_in, l_in = r.backward_inputs(tdt)
    o_in, l_in = _place(o_in, dev, off), l_in.contiguous()
    B, T, H, hd = c.B, c.T, c.H, c.hd
    out, lse = _launch3(f"{what} forward", dev, [((B, T, H * hd), tdt, True), ((B, H, T), torch.float32, False)],
                        lambda o, l: check(lib.mae_attention_fwd(_ptr(q), B, T, H, hd, dt, _ptr(o), _ptr(l), s)), off)
    (dqkv,) = _launch3(f"{what} backward", dev, [((B, T, 3 * H * hd), tdt, True)],
                       lambda d: check(lib.mae_attention_bwd(_ptr(q), _ptr(o_in), _ptr(g), _ptr(l_in), B, T, H, hd, dt, _ptr(d), s)), off)
    return out, lse, dqkv


def _settle(c, family, reps, fails):
    rt = c.route
    for k, rep in reps.items():
        lbl = (rt.fwd.label if k in ("out", "lse") else rt.bwd.label, k)
        if lbl not in WORST or rep.worst_ratio > WORST[lbl][0]:
            WORST[lbl] = (rep.worst_ratio, c.id, family)
        if not rep.ok:
            fails.append(f"{c.id} [{family}] {c.label}: {rep}")
    print(c.id, family, {k: f"{rep.worst_ratio:.3f}" for k, rep in reps.items()})


def _exact(c, family, name, got, want, fails):
    n = R.exact_mismatches(got, want)
    EXACT["checked"] += got.numel()
    EXACT["differing"] += n
    if n:
        i = (_bits(got.contiguous()) != _bits(want.contiguous())).nonzero()[0].tolist()
        fails.append(f"{c.id} [{family}] {c.label}: {name} differs in {n} of {got.numel()} elements, first at {i}")


@pytest.mark.parametrize("cid", list(CASES))
def test_attention_per_element(dev, cid):
    c = CASES[cid]
    rt, (dt, tdt), fails = c.route, DT[c.dtype], []
    for sigma in (1, 3):
        qkv, do = (x.to(dev) for x in R.gen_random(c, sigma, tdt))
        r = R.reference(qkv, do, c.H, c.hd)
        out, lse, dqkv = _run(c, dev, qkv, do, r, f"{cid} sigma={sigma}")
        _settle(c, f"sigma={sigma}", {**R.check_fwd(r, rt.fwd, out, lse), **R.check_bwd(r, rt.bwd, dqkv)}, fails)

    qkv, do, sigma, want_out, want_dv, lse_exact = R.gen_routing(c, tdt)
    qkv, do, want_out, want_dv = (x.to(dev) for x in (qkv, do, want_out, want_dv))
    r = R.reference(qkv, do, c.H, c.hd)
    out, lse, dqkv = _run(c, dev, qkv, do, r, f"{cid} routing")
    _exact(c, "routing", "out = V[sigma]", out, want_out, fails)
    if c.dtype == "bf16":   # the recomputed P = 1 +- a few u32 |lse| rounds to 1 in bf16 (kernel or output); fp32 keeps it: the bound
        _exact(c, "routing", "dV = dO[sigma^-1]", R.split_heads(dqkv, c.H, c.hd, 3)[2].contiguous(), want_dv, fails)
    _settle(c, "routing", {**R.check_fwd(r, rt.fwd, out, lse), **R.check_bwd(r, rt.bwd, dqkv)}, fails)

    qkv, count = R.gen_counting(c, tdt)
    qkv = qkv.to(dev)
    do = torch.zeros(c.B, c.T, c.H * c.hd, dtype=tdt, device=dev)
    r = R.reference(qkv, do, c.H, c.hd)
    out, lse, dqkv = _run(c, dev, qkv, do, r, f"{cid} counting")
    _settle(c, "counting", R.check_counting(r, rt.fwd, out, lse, count), fails)
    if int(R.at_fill(dqkv).sum()):
        fails.append(f"{cid} [counting]: d_qkv keeps fill values")
    assert not fails, "\n".join(fails)


def test_every_route_has_a_case():
    assert R.coverage_gaps() == []


def test_zz_report():
    table = {}
    for c in R.cases():
        table.setdefault(c.route.label, []).append(c)
    print(f"\nattention routes ({len(table)} labels, {len(CASES)} cases): forward | backward -> cases, lengths, B H mod 8")
    for lbl in sorted(table, key=str):
        v = table[lbl]
        print(f"  {' '.join(lbl):110s} {len(v):3d}  T={sorted({c.T for c in v})}  BHmod8={sorted({c.B * c.H % 8 for c in v})}")
    print(f"unreachable: {R.UNREACHABLE}")
    print("worst error / bound per kernel label and output:")
    for (lbl, k), (ratio, cid, fam) in sorted(WORST.items(), key=str):
        print(f"  {' '.join(lbl):70s} {k:4s} {ratio:.3f}  ({cid}, {fam})")
    print(f"exact outputs: {EXACT['differing']} differing of {EXACT['checked']} elements")
    if WORST:
        assert all(v[0] < 1 for v in WORST.values()) and EXACT["differing"] == 0
