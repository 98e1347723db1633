"""LayerNorm forward / backward and the column reductions behind dgamma / dbeta (k_layernorm.hip, sum_partials in k_patch.hip)
through the C ABI against tests/ln_ref.py, per element (-m gpu).

Every case of ln_ref.cases(): the eight selectable (lanes per row, vectors per lane) pairs at their smallest and largest dim, for
fp32 and bf16, at row counts that leave lane groups without a row, fill one block, start a second, give the backward 33 blocks,
and make the forward or the backward grid-stride loop take a second trip; with and without the fused add, a row map, accumulation
and dx_copy.  Outputs are NaN-filled with guard rows behind them, two launches must agree bit for bit, nothing outside the mapped
rows may change, and every element of y, mean, rstd, x_out, dx, dx_copy, dgamma and dbeta lies inside a bound counted from the
kernel's roundings (ln_ref's docstring).  The exactness cases (small integers) must come out bit-exact.  The last test runs a
66-LayerNorm MAE, whose backward overflows the 64-entry table of deferred second stages, against the oracle per named tensor.

The backward is given the float64 statistics rounded to fp32, not the forward kernel's, so each kernel is judged on its own.
The whole file (379 tests) takes about 10 s on an MI355X; the largest case 0.8 s."""
import numpy as np
import pytest
import torch

from oracle import mae_oracle as O
from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
from tests import ln_ref as R
from tests.util import BF16, F32, TDT, _ptr, check, lib, rel_err, stream

pytestmark = pytest.mark.gpu

CASES = R.cases()
BY_ID = {c.id: c for c in CASES}
GUARD_ROWS = 8
WORST = {}   # (instantiation, output) -> (worst error / bound, case id)


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.synchronize()


def _dt(c):
    return BF16 if c.dtype == "bf16" else F32


def put(a, dev, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev).to(dtype)


class Out:
    """rows x dim (dim = 0: a vector of ``rows``) on the device, NaN-filled or loaded with ``init``, GUARD_ROWS NaN rows behind it."""

    def __init__(self, rows, dim, dtype, dev, init=None):
        self.rows = rows
        shape = (rows + GUARD_ROWS, dim) if dim else (rows + GUARD_ROWS * 16,)
        self.full = torch.full(shape, float("nan"), dtype=dtype, device=dev)
        self.data = self.full[:rows]
        if init is not None:
            self.data.copy_(torch.from_numpy(init))

    def host(self):
        return self.data.float().cpu().numpy()

    def bits(self):
        return self.full.view(torch.int32 if self.full.dtype == torch.float32 else torch.int16)

    def guard_intact(self):
        return bool(torch.isnan(self.full[self.rows:].float()).all())


def _same_and_guarded(a, b, what):
    torch.cuda.synchronize()
    for k in a:
        if a[k] is not None:
            assert a[k].guard_intact() and b[k].guard_intact(), f"{what}: guard rows of {k} were written"
            assert torch.equal(a[k].bits(), b[k].bits()), f"{what}: two launches differ in {k}"


def run_fwd(c, d, dev):
    """Two launches into separate NaN-filled outputs -> (out dict for ln_ref.check_fwd, x_out before the launch)."""
    dt, tdt = _dt(c), TDT[_dt(c)]
    x, gamma, beta = put(d["x"], dev), put(d["gamma"], dev), put(d["beta"], dev)
    branch, rmap = put(d["branch"], dev, tdt), put(d["row_map"], dev, torch.int32)
    sets = []
    for _ in range(2):
        o = dict(y=Out(c.rows, c.dim, tdt, dev), mean=Out(c.rows, 0, torch.float32, dev), rstd=Out(c.rows, 0, torch.float32, dev),
                 x_out=Out(c.src_rows, c.dim, torch.float32, dev) if c.add else None)
        if c.add:
            check(lib.mae_add_layernorm_fwd(_ptr(x), _ptr(branch), _ptr(o["x_out"].full), _ptr(rmap) if c.map else None, _ptr(gamma), _ptr(beta),
                                            R.EPS, c.rows, c.dim, dt, _ptr(o["y"].full), _ptr(o["mean"].full), _ptr(o["rstd"].full), stream(dev)))
        else:
            check(lib.mae_layernorm_fwd(_ptr(x), _ptr(rmap) if c.map else None, _ptr(gamma), _ptr(beta), R.EPS, c.rows, c.dim, dt,
                                        _ptr(o["y"].full), _ptr(o["mean"].full), _ptr(o["rstd"].full), stream(dev)))
        sets.append(o)
    _same_and_guarded(sets[0], sets[1], f"{c.id} forward")
    out = {k: (v.host() if v is not None else None) for k, v in sets[0].items()}
    return out, (np.full((c.src_rows, c.dim), np.nan, np.float32) if c.add else None)


def run_bwd(c, d, mean, rstd, dev):
    """Two launches -> (out dict for ln_ref.check_bwd, dx before the launch).  partial holds exactly the 2 G dim floats the launch may use."""
    dt, tdt, geo = _dt(c), TDT[_dt(c)], c.geo
    x, gamma, dy = put(d["x"], dev), put(d["gamma"], dev), put(d["dy"], dev, tdt)
    mu, rs, rmap = put(mean, dev), put(rstd, dev), put(d["row_map"], dev, torch.int32)
    init = d["res"] if c.accumulate else np.full((c.src_rows, c.dim), np.nan, np.float32)
    sets = []
    for _ in range(2):
        o = dict(dx=Out(c.src_rows, c.dim, torch.float32, dev, init if c.accumulate else None),
                 dx_copy=Out(c.src_rows, c.dim, tdt, dev) if c.copy else None, dgamma=Out(c.dim, 0, torch.float32, dev),
                 dbeta=Out(c.dim, 0, torch.float32, dev), partial=Out(2 * geo.bwd_grid * c.dim, 0, torch.float32, dev))
        check(lib.mae_layernorm_bwd(_ptr(dy), dt, _ptr(x), _ptr(rmap) if c.map else None, _ptr(gamma), _ptr(mu), _ptr(rs), c.rows, c.dim,
                                    c.accumulate, _ptr(o["dx"].full), _ptr(o["dx_copy"].full) if c.copy else None, _ptr(o["dgamma"].full),
                                    _ptr(o["dbeta"].full), _ptr(o["partial"].full), stream(dev)))
        sets.append(o)
    _same_and_guarded(sets[0], sets[1], f"{c.id} backward")
    out = {k: (v.host() if v is not None else None) for k, v in sets[0].items()}
    assert np.isfinite(out["partial"]).all(), f"{c.id}: the first stage left part of partial[G][2][dim] unwritten"
    return out, init


def note(c, ratios):
    for k, v in ratios.items():
        key = (c.label if k in ("y", "mean", "rstd") else c.label.replace(f"ADD {int(c.add)}, ", ""), k)
        if key not in WORST or v > WORST[key][0]:
            WORST[key] = (v, c.id)


def test_case_table_is_complete():
    assert R.coverage_gaps(CASES) == []


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_layernorm_per_element(dev, cid):
    c = BY_ID[cid]
    d = R.gen_case(c)
    out, init = run_fwd(c, d, dev)
    ratios, fails = R.check_fwd(c, d, out, init)
    mean, rstd = R.bwd_stats(c, d)
    out, init = run_bwd(c, d, mean, rstd, dev)
    r2, f2 = R.check_bwd(c, d, mean, rstd, out, init)
    ratios.update(r2)
    print(cid, c.label, {k: f"{v:.3f}" for k, v in ratios.items()})
    note(c, ratios)
    assert not fails + f2, "\n".join([cid, c.label] + fails + f2)


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_layernorm_exact_on_small_integers(dev, cid):
    """dgamma / dbeta equal the float64 sums bit for bit at every dim (33 blocks and both wraps included); at power-of-two dims so do dx,
    dx_copy (after its bf16 rounding) and the forward mean; x_out = fl32(x + branch) always."""
    c = BY_ID[cid]
    d = R.gen_exact(c)
    out, _ = run_fwd(c, d, dev)
    fails = R.check_exact_fwd(c, d, out)
    out, init = run_bwd(c, d, d["mean"], d["rstd"], dev)
    _, f2 = R.check_bwd(c, d, d["mean"], d["rstd"], out, init, exact=True)
    assert not fails + f2, "\n".join([cid, c.label] + fails + f2)


# ------------------------------------------------------------------------------------------------ the deferred second stages
DEEP = O.MAEConfig(image_size=16, patch_size=4, in_chans=3, embed_dim=32, depth=31, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                   decoder_num_heads=2)
DEEP_TOL = 3e-4   # the fp32 figure of test_other_geometries_match_oracle; the fp32 oracle itself is within 9.1e-7 of the float64 oracle for every
                  # tensor compared here (measured on the CPU at this depth), so the figure is not widened


def _deep_model(dev):
    params = O.init_params(DEEP, 73)
    O.randomize_params(params)
    model = MaskedAutoencoder(dict(image_size=16, patch_size=4, in_chans=3, mask_ratio=0.75, engine_precision="fp32"),
                              dict(embed_dim=32, depth=31, num_heads=2), dict(decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2))
    model.load_state_dict(params, strict=True)
    return model.to(dev), params


def test_more_than_64_layernorms_in_one_backward(dev, monkeypatch):
    """31 encoder blocks + 1 decoder block = 66 LayerNorms: the table of deferred dgamma / dbeta reductions is flushed in the middle of the
    backward and its partial slots are reused.  The gradient of every LayerNorm weight and bias, of the class token and of the mask token
    matches the oracle tensor by tensor, also with the weight gradients of a block launched apart (MAE_WGRAD_PAIR=0)."""
    B = 2
    images = O.synthetic_images(B, DEEP)
    noise = O.make_noise(B, DEEP.sequence_length, torch.Generator().manual_seed(74))
    model, params = _deep_model(dev)
    loss_ref, grads_ref, aux = O.loss_and_grads(params, DEEP, images, noise, 0.75)
    names = [n for n in grads_ref if "norm" in n] + ["encoder.vit.cls_token", "decoder.mask_token"]
    assert len(names) == 2 * 66 + 2
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    errs = {n: rel_err(g[n], grads_ref[n]) for n in names}
    worst = max(errs, key=errs.get)
    print(f"worst of {len(names)} tensors: {worst} {errs[worst]:.3e}")
    assert all(float(grads_ref[n].norm()) > 0 for n in names)
    bad = {n: e for n, e in errs.items() if not e < DEEP_TOL}
    assert not bad, bad
    monkeypatch.setenv("MAE_WGRAD_PAIR", "0")   # the A/B switch of k_gemm_tn.hip: every weight gradient in a launch of its own
    m, _ = _deep_model(dev)
    m.loss_and_grads(images.to(dev), noise.to(dev))
    torch.cuda.synchronize()
    gs = m.named_flat_views(m.flat_grads.clone().cpu())
    assert all(rel_err(gs[n], grads_ref[n]) < DEEP_TOL for n in names)


def test_zz_report():
    """Prints the worst error / bound per instantiation and output over the cases that ran."""
    print("\nworst error / bound per instantiation and output:")
    for (label, k), (ratio, cid) in sorted(WORST.items()):
        print(f"  {label:34s} {k:8s} {ratio:.3f}  ({cid})")
    assert all(v[0] <= 1.0 for v in WORST.values())
