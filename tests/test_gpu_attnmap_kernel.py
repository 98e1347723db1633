"""attn_colsum_kernel (k_attnmap.hip) through mae_attention_colsum alone, per element against fp64 (-m gpu).

Cases: tests/attnmap_ref.cases() -- every length of 1, 2, 17, 63, 64, 65, 128, 129, 145, 197, 257 and the kernel's limit with three head
widths each, head counts 1, 2, 3, 6, 16, batches 1, 3, 7 and both types, every pair of those covered.  Per case and input family
(sigma = 1, and "large" whose scaled scores pass +-100: without the row maximum the exponential overflows) five start weights: one-hot
at row 0 and at row T - 1, uniform, random non-negative with exact zeros, and the mixed row of the uniform call.  Every element of
per_head and mixed must lie within attnmap_ref.colsum_bound of the fp64 reference on the same stored inputs; the outputs sit between
guard bands that must keep their fill.  Further: a strided (B, 3, H, T) buffer written slice by slice, either output alone against both,
two runs, an image alone against the same image in a batch of 7 (all bit for bit), and refusals that must write nothing.
The last test prints the worst error / bound per kernel instance (-s).  About 6 s on an MI355X."""
import math

import pytest
import torch

from tests import attnmap_ref as R
from tests.attn_ref import at_fill, exact_mismatches, fill_like, guarded, guards_touched
from tests.util import _ptr, check, lib, stream

pytestmark = pytest.mark.gpu

DT = {"f32": 0, "bf16": 1}                    # MAE_F32, MAE_BF16
TD = {"f32": torch.float32, "bf16": torch.bfloat16}
WORST = {}


def max_tokens():
    vals = {lib.mae_attention_colsum_max_tokens(hd, dt) for hd in R.HDS for dt in (0, 1)}
    assert len(vals) == 1, vals
    return vals.pop()


def colsum(c, qkv, w, per_head, mixed, s, stride=None):
    check(lib.mae_attention_colsum(_ptr(qkv), DT[c.dtype], c.B, c.T, c.H, c.hd, _ptr(w), _ptr(per_head), c.H * c.T if stride is None else stride,
                                   _ptr(mixed), s))


def run(c, qkv, w, s, dev, want_head=True, want_mixed=True):
    """-> per_head (B, H, T), mixed (B, T) (None where not asked for); the guard bands are checked."""
    hb, head = guarded((c.B, c.H, c.T), torch.float32, dev) if want_head else (None, None)
    mb, mixed = guarded((c.B, c.T), torch.float32, dev) if want_mixed else (None, None)
    colsum(c, qkv, w, head, mixed, s)
    torch.cuda.synchronize()
    for buf, view in ((hb, head), (mb, mixed)):
        if buf is not None:
            assert guards_touched(buf, view) == 0, f"{c.id}: wrote outside its output"
            assert not bool(at_fill(view).any()), f"{c.id}: left output elements unwritten"
    return head, mixed


def judge(c, what, got, ref, e, fails):
    g = got.double()
    bad = ~torch.isfinite(g) | ((g - ref).abs() > e)
    ratio = float(torch.nan_to_num((g - ref).abs() / e, nan=float("inf")).max())
    key = c.route
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, f"{c.id} {what}")
    print(f"{c.id:28s} {what:34s} worst error / bound {ratio:.3f}")
    if bool(bad.any()):
        i = int(bad.flatten().to(torch.int32).argmax())
        fails.append(f"{c.id} {what}: {int(bad.sum())} of {g.numel()} outside the bound (first flat index {i}: got {float(g.flatten()[i]):.9g}, "
                     f"fp64 {float(ref.flatten()[i]):.9g}, allowed {float(e.flatten()[i]):.3g}); worst ratio {ratio:.3g}")


def test_limits_query():
    assert max_tokens() >= 257
    for hd, dt in ((20, 0), (64, 2), (0, 0), (128, 1)):
        assert lib.mae_attention_colsum_max_tokens(hd, dt) == -1


@pytest.mark.parametrize("c", R.cases(512), ids=lambda c: c.id)
def test_every_element_against_fp64(dev, c):
    assert max_tokens() == 512   # the table's last length is the kernel's limit
    s, fails = stream(dev), []
    for family in ("random", "large"):
        qkv = R.gen_qkv(c, family, TD[c.dtype]).to(dev)
        parts = R.probabilities(qkv, c.H, c.hd)
        if family == "large" and c.T >= 17:
            assert float(parts[0].abs().max()) > 100.0
        ws = {k: v.to(dev) for k, v in R.gen_weights(c).items()}
        for name in R.WEIGHTS:
            if name == "chained":   # the mixed row the uniform weight produced: what the second step of a rollout reads
                w = run(c, qkv, ws["uniform"], s, dev, want_head=False)[1].clone()
            else:
                w = ws[name]
            head, mixed = run(c, qkv, w, s, dev)
            ref_head = R.colsum_from(parts[1], w)
            e_head, e_mixed = R.colsum_bound(qkv, w, c.H, c.hd, parts)
            judge(c, f"{family} {name} per_head", head, ref_head, e_head, fails)
            judge(c, f"{family} {name} mixed", mixed, R.mixed_ref(w, ref_head), e_mixed, fails)
            if name.startswith("onehot"):   # a one-hot weight returns that row of P: its rows sum to 1
                assert float((head.double().sum(-1) - 1).abs().max()) <= 1e-5
    assert not fails, "\n".join(fails)


PROP = [R.Case("bf16", 7, 145, 6, 64), R.Case("f32", 7, 17, 3, 24), R.Case("f32", 7, 257, 2, 48), R.Case("bf16", 7, 65, 16, 16)]


@pytest.mark.parametrize("c", PROP, ids=lambda c: c.id)
def test_outputs_alone_runs_and_batches_agree_bit_for_bit(dev, c):
    s = stream(dev)
    qkv = R.gen_qkv(c, "random", TD[c.dtype]).to(dev)
    for name, w in R.gen_weights(c).items():
        w = w.to(dev)
        head, mixed = run(c, qkv, w, s, dev)
        head_only = run(c, qkv, w, s, dev, want_mixed=False)[0]
        mixed_only = run(c, qkv, w, s, dev, want_head=False)[1]
        assert exact_mismatches(head_only, head) == 0 and exact_mismatches(mixed_only, mixed) == 0, name
        again = run(c, qkv, w, s, dev)
        assert exact_mismatches(again[0], head) == 0 and exact_mismatches(again[1], mixed) == 0, name
        one = R.Case(c.dtype, 1, c.T, c.H, c.hd)
        for b in (0, 3, 6):   # the image alone: another grid, the same bits
            h1, m1 = run(one, qkv[b:b + 1].clone(), w[b:b + 1].clone(), s, dev)   # copies: 16-byte aligned whatever b T is
            assert exact_mismatches(h1[0], head[b]) == 0 and exact_mismatches(m1[0], mixed[b]) == 0, (name, b)


@pytest.mark.parametrize("c", [R.Case("f32", 3, 17, 3, 32), R.Case("bf16", 2, 129, 2, 64)], ids=lambda c: c.id)
def test_strided_slices(dev, c):
    """Slice i of a (B, 3, H, T) buffer, written in place, holds the bits of a packed call; nothing else changes.  H T = 51 floats at the
    first case: the slices are not 16-byte aligned."""
    s = stream(dev)
    qkv = R.gen_qkv(c, "random", TD[c.dtype]).to(dev)
    ws = [v.to(dev) for k, v in R.gen_weights(c).items() if k != "onehot_last"]
    buf, view = guarded((c.B, 3, c.H, c.T), torch.float32, dev)
    for i, w in enumerate(ws):
        before = view.clone()
        colsum(c, qkv, w, view[0, i], None, s, stride=3 * c.H * c.T)
        torch.cuda.synchronize()
        packed = run(c, qkv, w, s, dev, want_mixed=False)[0]
        assert exact_mismatches(view[:, i], packed) == 0, i
        others = [j for j in range(3) if j != i]
        assert exact_mismatches(view[:, others], before[:, others]) == 0, i
        assert guards_touched(buf, view) == 0
    assert not bool(at_fill(view).any())


def test_refused_calls_write_nothing(dev):
    s = stream(dev)
    top = max_tokens()
    c = R.Case("f32", 2, 17, 2, 16)
    big = R.Case("f32", 1, top + 1, 1, 16)
    qkv = torch.randn(1, top + 1, 3 * 17 * 20, device=dev)   # large enough for every shape below
    w = torch.full((2 * (top + 1),), 0.01, device=dev)
    hb, head = guarded((2 * 17 * (top + 1),), torch.float32, dev)
    mb, mixed = guarded((2 * (top + 1),), torch.float32, dev)

    def call(case=c, q=qkv, wt=w, ph=head, mx=mixed, stride=None, dtype=0):
        rc = lib.mae_attention_colsum(_ptr(q), dtype, case.B, case.T, case.H, case.hd, _ptr(wt), _ptr(ph), case.H * case.T if stride is None else stride,
                                      _ptr(mx), s)
        check(0)
        return rc, lib.mae_last_error().decode()

    w_before = w.clone()
    for kw, word in ((dict(case=big), str(top)), (dict(case=R.Case("f32", 2, 17, 2, 20)), "head_dim"), (dict(case=R.Case("f32", 2, 17, 17, 16)), "H = 17"),
                     (dict(case=R.Case("f32", 2, 0, 2, 16)), "positive"), (dict(wt=w[1:]), "aligned"), (dict(q=qkv.view(-1)[1:]), "aligned"),
                     (dict(mx=mixed[1:]), "aligned"), (dict(mx=w), "alias"), (dict(mx=w[16:]), "alias"), (dict(ph=None, mx=None), "both null"),
                     (dict(stride=2 * 17 - 1), "per_head_stride"), (dict(dtype=2), "dtype"), (dict(wt=None), "null")):
        rc, msg = call(**kw)
        assert rc != 0 and word in msg, (kw.keys(), msg)
    torch.cuda.synchronize()
    assert bool(at_fill(hb).all()) and bool(at_fill(mb).all()) and torch.equal(w, w_before)
    rc, msg = call()
    assert rc == 0, msg
    torch.cuda.synchronize()
    n = 2 * 2 * 17
    assert not bool(at_fill(head[:n]).any()) and bool(at_fill(head[n:]).all()) and guards_touched(hb, head) == 0
    assert not bool(at_fill(mixed[:2 * 17]).any()) and bool(at_fill(mixed[2 * 17:]).all()) and guards_touched(mb, mixed) == 0


def test_zz_print_worst_ratios():
    """Worst error / bound per kernel instance over the tests above."""
    for k in sorted(WORST):
        print(f"attn_colsum  {k:10s} {WORST[k][0]:.3f}  ({WORST[k][1]})")
    assert all(math.isfinite(v[0]) and v[0] <= 1.0 for v in WORST.values())
