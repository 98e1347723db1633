"""mae_probe_sweep_head and mae_lars_step_groups on the MI355X: every head against the fp64 restatement (tests/probe_sweep_ref.py) at the
shapes where the tiling can go wrong, the bits of a head independent of the stack it sits in, the optional outputs, the refusals, and the
grouped LARS step bit for bit against mae_lars_step per segment."""
import numpy as np
import pytest
import torch

from tests import probe_ref as R
from tests import probe_sweep_ref as S
from tests.util import rel_err

pytestmark = pytest.mark.gpu

POISON = 777.0
# (B, D, C, G): one row / the smallest of everything; HF padded, B below a tile, D no multiple of 8, heads straddling column tiles;
# more than one row tile; the largest D and C and more than one batch slice; the most heads
SHAPES = [(1, 4, 2, 1), (7, 148, 10, 3), (33, 384, 100, 5), (257, 1024, 128, 2), (64, 384, 10, 64)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


def labels_for(B, C, seed=0):
    return np.random.default_rng([B, C, seed, 3]).integers(0, C, B)


def run(dev, y, flat, C, labels=None, logits=True, grads=True, short_scratch=0, misalign=None, G=None, D=None):
    """One mae_probe_sweep_head call on numpy inputs: dict(rc, need, logits, loss, correct, grads) of numpy outputs; every output
    buffer starts poisoned, and one that is not passed (logits / grads = False) must come back so."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    B = y.shape[0]
    D = y.shape[1] if D is None else D
    G = flat.shape[0] if G is None else G
    yd, fd = torch.from_numpy(np.ascontiguousarray(y)).to(dev), torch.from_numpy(np.ascontiguousarray(flat)).to(dev)
    ld = None if labels is None else torch.from_numpy(np.asarray(labels, dtype=np.int64)).to(dev)
    gb = max(G, 1)
    lg = torch.full((gb, B, C), POISON, dtype=torch.float32, device=dev)
    loss = torch.full((gb + 4,), POISON, dtype=torch.float32, device=dev)
    correct = torch.full((gb + 4,), -7, dtype=torch.int32, device=dev)
    hg = torch.full((gb, S.head_floats(C, D)), POISON, dtype=torch.float32, device=dev)
    need = lib.mae_probe_sweep_scratch_bytes(B, D, C, G)
    nbytes = max(need, 1024) - short_scratch
    scratch = torch.empty(nbytes + 16, dtype=torch.uint8, device=dev)
    yp = yd.data_ptr() + (4 if misalign == "y" else 0)
    sp = scratch.data_ptr() + (4 if misalign == "scratch" else 0)
    rc = lib.mae_probe_sweep_head(yp, B, D, _ptr(fd), G, C, _ptr(ld), _ptr(lg) if logits else None, _ptr(loss), _ptr(correct),
                                  _ptr(hg) if grads else None, sp, nbytes, _stream(dev))
    torch.cuda.synchronize()
    return dict(rc=rc, need=need, logits=np_(lg), loss=np_(loss), correct=np_(correct), grads=np_(hg))


@pytest.mark.parametrize("B,D,C,G", SHAPES)
def test_heads_against_fp64(dev, B, D, C, G):
    y = S.gen_rows(B, D)
    W, b = S.gen_heads(G, C, D)
    labels = labels_for(B, C)
    out = run(dev, y, S.pack(W, b), C, labels)
    assert out["rc"] == 0
    ref = S.sweep_head(y, W, b, labels)
    nw, fails, worst = C * D, [], dict(logits=0.0, loss=0.0, dW=0.0, db=0.0)
    for g in range(G):
        ratio, i = R.worst(out["logits"][g], ref[g]["logits"], R.linear_bound(y, W[g], b[g]))
        errs = dict(logits=ratio, loss=abs(float(out["loss"][g]) - ref[g]["loss"]) / abs(ref[g]["loss"]),
                    dW=rel_err(torch.from_numpy(out["grads"][g, :nw]), torch.from_numpy(ref[g]["dW"].reshape(-1))),
                    db=rel_err(torch.from_numpy(out["grads"][g, nw:nw + C]), torch.from_numpy(ref[g]["db"])))
        for k, v in errs.items():
            worst[k] = max(worst[k], v)
            if not v <= (1.0 if k == "logits" else 1e-5):
                fails.append(f"head {g} {k}: {v:.3e}" + (f" at flat index {i}" if k == "logits" else ""))
        assert int(out["correct"][g]) == int((out["logits"][g].argmax(1) == labels).sum())   # exact on the GPU's own logits
        assert np.all(out["grads"][g, nw + C:] == 0.0)                                        # the padding is written as zeros
    print(f"({B}, {D}, {C}, {G}): logits worst error / bound {worst['logits']:.3g}; worst rel_err loss {worst['loss']:.3e} "
          f"dW {worst['dW']:.3e} db {worst['db']:.3e}")
    assert np.all(out["loss"][G:] == POISON) and np.all(out["correct"][G:] == -7)
    assert not fails, "\n".join(fails)


# rows 257: three batch slices in the weight gradient; C = 100: heads that straddle the 32- and 128-column tiles
@pytest.mark.parametrize("B,D,C", [(7, 148, 10), (33, 384, 100), (257, 64, 10)])
def test_a_heads_bits_do_not_depend_on_the_stack(dev, B, D, C):
    G = 5
    y = S.gen_rows(B, D, seed=1)
    W, b = S.gen_heads(G, C, D, seed=1)
    W[3], b[3] = W[1].copy(), b[1].copy()   # two identical heads in one stack
    labels = labels_for(B, C, seed=1)
    full = run(dev, y, S.pack(W, b), C, labels)
    again = run(dev, y, S.pack(W, b), C, labels)
    assert full["rc"] == 0 and again["rc"] == 0
    keys = ("logits", "loss", "correct", "grads")
    for k in keys:
        assert np.array_equal(full[k], again[k]), f"{k}: a repeated call differs"
        assert np.array_equal(full[k][1], full[k][3]), f"{k}: identical heads at positions 1 and 3 differ"
    for g in (0, 2, 4):   # first, middle, last
        alone = run(dev, y, S.pack(W[g:g + 1], b[g:g + 1]), C, labels)
        assert alone["rc"] == 0
        for k in keys:
            assert np.array_equal(full[k][g], alone[k][0]), f"{k}: head {g} of {G} differs from the same head alone"
    assert np.isfinite(full["grads"]).all() and np.abs(full["grads"]).max() > 0


def test_optional_outputs(dev):
    B, D, C, G = 33, 148, 10, 3
    y = S.gen_rows(B, D, seed=2)
    W, b = S.gen_heads(G, C, D, seed=2)
    labels = labels_for(B, C, seed=2)
    flat = S.pack(W, b)
    full = run(dev, y, flat, C, labels)
    ev = run(dev, y, flat, C, labels, grads=False)            # the evaluation call: the gradient buffer stays poisoned
    assert ev["rc"] == 0 and np.all(ev["grads"] == POISON)
    for k in ("logits", "loss", "correct"):
        assert np.array_equal(ev[k], full[k])
    nol = run(dev, y, flat, C, labels, logits=False)          # the logits stay in the scratch
    assert nol["rc"] == 0 and np.all(nol["logits"] == POISON)
    for k in ("loss", "correct", "grads"):
        assert np.array_equal(nol[k], full[k])
    fwd = run(dev, y, flat, C, None, grads=False)             # no labels: logits only
    assert fwd["rc"] == 0 and np.array_equal(fwd["logits"], full["logits"])
    assert np.all(fwd["loss"] == POISON) and np.all(fwd["correct"] == -7) and np.all(fwd["grads"] == POISON)


def test_label_out_of_range(dev):
    """classifier_head_kernel's rule: never an index; the row's loss and dlogits are NaN, the row is not correct."""
    B, D, C, G = 7, 148, 10, 2
    y = S.gen_rows(B, D, seed=3)
    W, b = S.gen_heads(G, C, D, seed=3)
    labels = labels_for(B, C, seed=3)
    good = run(dev, y, S.pack(W, b), C, labels)
    labels[2] = C
    bad = run(dev, y, S.pack(W, b), C, labels)
    assert bad["rc"] == 0 and np.array_equal(bad["logits"], good["logits"])
    assert np.isnan(bad["loss"][:G]).all() and np.isnan(bad["grads"][:, :C * D + C]).all() and np.all(bad["grads"][:, C * D + C:] == 0.0)
    for g in range(G):
        assert int(bad["correct"][g]) == int((good["logits"][g].argmax(1) == labels).sum())


@pytest.mark.parametrize("what", ["G=0", "G=65", "C=1", "C=129", "D=6", "D=1028", "misaligned y", "misaligned scratch", "short scratch"])
def test_refusals_write_nothing(dev, what):
    from ssrl_vit_mae_jepa_amd._lib import lib
    B, D, C, G = 8, 16, 4, 2
    kw = {}
    if what.startswith("G="):
        G = int(what[2:])
    elif what.startswith("C="):
        C = int(what[2:])
    elif what.startswith("D="):
        D = int(what[2:])
    elif what.startswith("misaligned"):
        kw["misalign"] = what.split()[1]
    else:
        kw["short_scratch"] = 16
    y = np.zeros((B, max(D, 16)), dtype=np.float32)                 # a refused call reads nothing: the buffers only have to exist
    flat = np.zeros((max(G, 1), S.head_floats(max(C, 2), max(D, 16))), dtype=np.float32)
    out = run(dev, y, flat, C, labels_for(B, max(C, 2)), G=G, D=D, **kw)
    assert out["rc"] != 0 and lib.mae_last_error()
    assert np.all(out["logits"] == POISON) and np.all(out["loss"] == POISON) and np.all(out["correct"] == -7) and np.all(out["grads"] == POISON)
    if what[0] in "GCD":
        assert out["need"] == -1 and lib.mae_probe_sweep_scratch_bytes(B, D, C, G) == -1
    assert lib.mae_probe_sweep_scratch_bytes(0, 16, 4, 2) == -1 and lib.mae_probe_sweep_scratch_bytes(2 ** 31 // 8, 16, 4, 2) == -1
    assert lib.mae_probe_sweep_scratch_bytes(2 ** 31 // 8 - 1, 16, 4, 2) > 0


# ------------------------------------------------------------------------------------------------------------------
# mae_lars_step_groups
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adapt", [1, 0])
@pytest.mark.parametrize("G,count", [(1, 4), (3, 1480), (64, 38400), (3, 38400), (64, 4)])
def test_lars_groups_equal_lars_per_segment(dev, G, count, adapt):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    stride = count + 8   # a gap between the groups
    mom, tc = 0.9, 0.001
    r = np.random.default_rng([G, count, adapt])
    lr = (0.05 * 2.0 ** r.integers(0, 6, G)).astype(np.float32)
    wd = np.where(np.arange(G) % 2 == 0, 0.0, 10.0 ** r.uniform(-4, -2, G)).astype(np.float32)   # 0 included
    p, g, mu = (np.full(G * stride, POISON, dtype=np.float32) for _ in range(3))
    for i in range(G):
        a, b, c = R.gen_lars(count, seed=i, zero_p=(i == G - 1 and G > 1))   # one all-zero-parameter group: q = 1
        p[i * stride:i * stride + count], g[i * stride:i * stride + count], mu[i * stride:i * stride + count] = a, b, c
    s = _stream(dev)
    # the yardstick: mae_lars_step on each segment alone
    want_p, want_mu, want_n = p.copy(), mu.copy(), np.zeros((G, 2), dtype=np.float32)
    scratch1 = torch.empty(4096, dtype=torch.float32, device=dev)
    for i in range(G):
        sl = slice(i * stride, i * stride + count)
        pd, gd, md = (torch.from_numpy(x[sl].copy()).to(dev) for x in (p, g, mu))
        nd = torch.zeros(2, dtype=torch.float32, device=dev)
        check(lib.mae_lars_step(_ptr(pd), _ptr(gd), _ptr(md), count, adapt, float(lr[i]), mom, float(wd[i]), tc, _ptr(nd), _ptr(scratch1), s))
        torch.cuda.synchronize()
        want_p[sl], want_mu[sl], want_n[i] = np_(pd), np_(md), np_(nd)
    pd, gd, md = (torch.from_numpy(x.copy()).to(dev) for x in (p, g, mu))
    nd = torch.zeros(G, 2, dtype=torch.float32, device=dev)
    scratch = torch.empty(G * 4096, dtype=torch.float32, device=dev)
    check(lib.mae_lars_step_groups(_ptr(pd), _ptr(gd), _ptr(md), G, stride, count, adapt, lr.ctypes.data, wd.ctypes.data, mom, tc, _ptr(nd),
                                   _ptr(scratch), scratch.numel(), s))
    torch.cuda.synchronize()
    assert np.array_equal(np_(pd), want_p) and np.array_equal(np_(md), want_mu) and np.array_equal(np_(nd), want_n)   # the gaps included
    assert np.array_equal(np_(gd), g)
    assert not np.array_equal(want_p, p)
    # without norms_out: the same parameters
    pd2, md2 = torch.from_numpy(p.copy()).to(dev), torch.from_numpy(mu.copy()).to(dev)
    check(lib.mae_lars_step_groups(_ptr(pd2), _ptr(gd), _ptr(md2), G, stride, count, adapt, lr.ctypes.data, wd.ctypes.data, mom, tc, None,
                                   _ptr(scratch), scratch.numel(), s))
    torch.cuda.synchronize()
    assert np.array_equal(np_(pd2), want_p) and np.array_equal(np_(md2), want_mu)
    # refusals: too many groups, a short scratch, a stride that is no multiple of 4
    before = np_(pd2).copy()
    for args in ((65, stride, count, scratch.numel()), (G, stride, count, G * 4096 - 1), (G, stride + 2, count, scratch.numel())):
        rc = lib.mae_lars_step_groups(_ptr(pd2), _ptr(gd), _ptr(md2), args[0], args[1], args[2], adapt, lr.ctypes.data, wd.ctypes.data, mom, tc,
                                      None, _ptr(scratch), args[3], s)
        assert rc != 0
    torch.cuda.synchronize()
    assert np.array_equal(np_(pd2), before)
