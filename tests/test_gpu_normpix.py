"""Normalised-pixel targets on the GPU (-m gpu), kernel level: mae_patchify_gather_norm, mae_mse_loss_norm_pix and
mae_norm_pix_restore against the float64 reference of tests/normpix_ref.py.

Tolerances.  Target, per element: |got - ref| <= 2^-20 * (rstd_row + |ref|) (normpix_ref.bound: ~16 fp32 roundings of the centred
value, multiplied by rstd, plus a few ulps of rstd).  Loss: 1e-5 relative (an fp32 mean of up to ~5e5 non-negative terms in two
stages).  d_pred fp32: the target bound times 2 grad_scale / n plus 2^-22 relative (the subtraction of pred and the scaling);
d_pred bf16: one bf16 rounding (2^-8 relative) of the fp32 d_pred.  Restore: 2^-20 * (1 + |x|).  Every test prints the largest
observed error as a fraction of its bound."""
import functools
import math

import pytest
import torch

from ssrl_vit_mae_jepa_amd import _lib
from ssrl_vit_mae_jepa_amd._lib import check, lib
from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream, restore_pixels
from tests import normpix_ref as NR

pytestmark = pytest.mark.gpu

B = 3
# (image, patch, C, dtypes)
CASES = [(16, 4, 3, ("u8", "f32")),    # P = 48: fewer elements than lanes
         (32, 8, 3, ("u8", "f32")),    # P = 192: the product's patch
         (32, 8, 1, ("u8", "f32")),    # P = 64
         (12, 6, 3, ("f32",)),         # P = 108: patch no multiple of 4
         (28, 14, 3, ("f32",))]        # P = 588: no multiple of 64
PARAMS = [pytest.param(S, p, C_, dt, id=f"S{S}_p{p}_C{C_}_{dt}") for S, p, C_, dts in CASES for dt in dts]
MASKS = ("one", "rows", "most")
CONST, ONE_OFF = 1, 2   # image 1 is a constant 37; every patch of image 2 is a constant 100 with one pixel at 101


def make_images(S, p, C_, batch, g: torch.Generator) -> torch.Tensor:
    img = torch.randint(0, 256, (batch, C_, S, S), generator=g, dtype=torch.uint8)
    img[CONST] = 37
    img[ONE_OFF] = 100
    G = S // p
    for n in range(G * G):
        img[ONE_OFF, n % C_, (n // G) * p + n % p, (n % G) * p + (3 * n) % p] = 101
    return img


def make_indices(kind: str, G: int, batch: int, g: torch.Generator) -> torch.Tensor:
    """Token ids (patch + 1), distinct per image, in shuffled order.  "one": m = 1; "most": m = L - 2 = every patch but one;
    "rows": every token of patch row 1, one token of each later row and none of row 0."""
    N = G * G
    rows = []
    for b in range(batch):
        if kind == "one":
            pick = torch.randperm(N, generator=g)[:1]
        elif kind == "most":
            pick = torch.randperm(N, generator=g)[:N - 1]
        else:
            pick = torch.tensor(list(range(G, 2 * G)) + [r * G + (r + b) % G for r in range(2, G)])
            pick = pick[torch.randperm(pick.numel(), generator=g)]
        rows.append(pick + 1)
    return torch.stack(rows)


@functools.lru_cache(maxsize=None)
def case(S, p, C_, kind, batch=B):
    """One seeded problem and its float64 reference, computed once and shared by the tests (never modified)."""
    g = torch.Generator().manual_seed(4000 + 11 * S + p + 5 * C_ + MASKS.index(kind) + batch)
    u8 = make_images(S, p, C_, batch, g)
    idx = make_indices(kind, S // p, batch, g)
    if kind == "rows":
        band = (idx - 1) // (S // p)
        assert not (band == 0).any() and all(int((band[b] == 1).sum()) == S // p for b in range(batch))
    t, mean, rstd = NR.target_ref(u8, idx, p)
    pred = torch.randn(batch, idx.shape[1], p * p * C_, generator=g) * 0.9
    return dict(u8=u8, f32=NR.normalize_u8(u8), idx=idx, t=t, mean=mean, rstd=rstd, x=NR.patches_ref(u8, idx, p), pred=pred,
                bound=NR.bound(t, rstd))


def gather_norm(dev, images, idx, p, stats=True):
    images, idx = images.to(dev).contiguous(), idx.to(dev).contiguous()
    Bn, C_, S, _ = images.shape
    m = idx.shape[1]
    t = torch.empty(Bn, m, p * p * C_, dtype=torch.float32, device=dev)
    mean = torch.empty(Bn, m, dtype=torch.float32, device=dev) if stats else None
    rstd = torch.empty(Bn, m, dtype=torch.float32, device=dev) if stats else None
    check(lib.mae_patchify_gather_norm(_ptr(images), _lib.MAE_U8 if images.dtype == torch.uint8 else _lib.MAE_F32, _ptr(idx, torch.int64), Bn, C_, S,
                                       p, m, _ptr(t), _ptr(mean), _ptr(rstd), _stream(dev)))
    return t, mean, rstd


def gather_plain(dev, images, idx, p):
    images, idx = images.to(dev).contiguous(), idx.to(dev).contiguous()
    Bn, C_, S, _ = images.shape
    m = idx.shape[1]
    t = torch.empty(Bn, m, p * p * C_, dtype=torch.float32, device=dev)
    check(lib.mae_patchify_gather(_ptr(images), _lib.MAE_U8 if images.dtype == torch.uint8 else _lib.MAE_F32, _ptr(idx, torch.int64), Bn, C_, S, p, m,
                                  _ptr(t), _stream(dev)))
    return t


def mse_norm(dev, pred, images, idx, p, grad_scale, d_dtype):
    pred, images, idx = pred.to(dev).contiguous(), images.to(dev).contiguous(), idx.to(dev).contiguous()
    Bn, C_, S, _ = images.shape
    m = idx.shape[1]
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    scratch = torch.zeros(4096, dtype=torch.float32, device=dev)
    d = None if d_dtype is None else torch.empty(pred.shape, dtype=d_dtype, device=dev)
    check(lib.mae_mse_loss_norm_pix(_ptr(pred), _ptr(images), _lib.MAE_U8 if images.dtype == torch.uint8 else _lib.MAE_F32, _ptr(idx, torch.int64), Bn,
                                    C_, S, p, m, float(grad_scale), _ptr(loss), _ptr(d), _lib.MAE_BF16 if d_dtype == torch.bfloat16 else _lib.MAE_F32,
                                    _ptr(scratch), _stream(dev)))
    return loss, d


def ratio(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor) -> float:
    return float(((got.double().cpu() - ref).abs() / bound).max())


@pytest.mark.parametrize("S,p,C_,dt", PARAMS)
def test_gather_norm_matches_fp64(dev, S, p, C_, dt):
    worst = 0.0
    for kind in MASKS:
        c = case(S, p, C_, kind)
        t, mean, rstd = gather_norm(dev, c[dt], c["idx"], p)
        r = ratio(t, c["t"], c["bound"])
        worst = max(worst, r)
        print(f"gather_norm S{S} p{p} C{C_} {dt} {kind}: max error / bound = {r:.4f}")
        assert r <= 1.0, (kind, r)
        assert ((mean.double().cpu() - c["mean"]).abs() <= 2.0 ** -20).all()
        assert ((rstd.double().cpu() - c["rstd"]).abs() <= 2.0 ** -20 * c["rstd"]).all()
        # the constant image: exactly zero, rstd = fp32(1 / sqrt(1e-6))
        assert torch.equal(t[CONST], torch.zeros_like(t[CONST]))
        assert torch.equal(rstd[CONST].cpu(), torch.full_like(rstd[CONST].cpu(), float(torch.tensor(1.0 / math.sqrt(1e-6), dtype=torch.float64).float())))
        assert float(rstd[CONST][0]) == 1000.0
        # one pixel one level off: P - 1 equal values and one different, nothing flushed to zero
        assert (t[ONE_OFF].abs() > 0).all() and (t[ONE_OFF] > 1).sum() == t.shape[1]
        # NULL statistics outputs
        assert torch.equal(gather_norm(dev, c[dt], c["idx"], p, stats=False)[0], t)
    print(f"gather_norm S{S} p{p} C{C_} {dt}: WORST error / bound = {worst:.4f}")


@pytest.mark.parametrize("S,p,C_", [(S, p, C_) for S, p, C_, dts in CASES if "u8" in dts])
def test_uint8_and_fp32_routes_agree(dev, S, p, C_):
    for kind in MASKS:
        c = case(S, p, C_, kind)
        a, b = gather_norm(dev, c["u8"], c["idx"], p)[0], gather_norm(dev, c["f32"], c["idx"], p)[0]
        r = ratio(a, b.double().cpu(), c["bound"])
        print(f"u8 vs f32 S{S} p{p} C{C_} {kind}: max difference / bound = {r:.4f}")
        assert r <= 1.0
        la, lb = (mse_norm(dev, c["pred"], c[k], c["idx"], p, 1.0, None)[0].item() for k in ("u8", "f32"))
        assert abs(la - lb) <= 1e-5 * abs(lb)


@pytest.mark.parametrize("S,p,C_,dt", PARAMS)
def test_fused_loss_matches_fp64(dev, S, p, C_, dt):
    gs = 0.7
    for kind in MASKS:
        c = case(S, p, C_, kind)
        n = c["pred"].numel()
        loss_ref, d_ref = NR.loss_ref(c["pred"], c["u8"], c["idx"], p, grad_scale=gs)
        loss, d32 = mse_norm(dev, c["pred"], c[dt], c["idx"], p, gs, torch.float32)
        rel = abs(loss.item() - loss_ref) / loss_ref
        tol = c["bound"] * (2 * gs / n) + 2.0 ** -22 * d_ref.abs()
        r = ratio(d32, d_ref, tol)
        print(f"mse_norm_pix S{S} p{p} C{C_} {dt} {kind}: loss rel err {rel:.3e} (1e-5), d_pred max error / bound = {r:.4f}")
        assert rel <= 1e-5 and r <= 1.0, (kind, rel, r)
        loss_b, dbf = mse_norm(dev, c["pred"], c[dt], c["idx"], p, gs, torch.bfloat16)
        assert torch.equal(loss_b, loss)
        assert ((dbf.float() - d32).abs() <= 2.0 ** -8 * d32.abs() + 1e-38).all()
        loss_n, none = mse_norm(dev, c["pred"], c[dt], c["idx"], p, gs, None)   # d_pred may be NULL
        assert none is None and torch.equal(loss_n, loss)


@pytest.mark.parametrize("S,p,C_,dt", PARAMS)
def test_restore_inverts_the_standardisation(dev, S, p, C_, dt):
    for kind in MASKS:
        c = case(S, p, C_, kind)
        t = gather_norm(dev, c[dt], c["idx"], p)[0]
        x = gather_plain(dev, c[dt], c["idx"], p)
        assert torch.equal(x.double().cpu(), c["x"])   # mae_patchify_gather itself is exact
        out = restore_pixels(c[dt].to(dev), t, c["idx"].to(dev), p)
        r = ratio(out, c["x"], 2.0 ** -20 * (1 + c["x"].abs()))
        print(f"restore S{S} p{p} C{C_} {dt} {kind}: max error / bound = {r:.4f}")
        assert r <= 1.0
        alias = t.clone()
        assert restore_pixels(c[dt].to(dev), alias, c["idx"].to(dev), p, out=alias) is alias and torch.equal(alias, out)


@pytest.mark.parametrize("S,p,C_,dt", PARAMS)
def test_runs_are_bit_identical_and_rows_do_not_depend_on_the_batch(dev, S, p, C_, dt):
    for kind in MASKS:
        c = case(S, p, C_, kind)
        img, idx = c[dt], c["idx"]
        t1, t2 = gather_norm(dev, img, idx, p), gather_norm(dev, img, idx, p)
        assert all(torch.equal(a, b) for a, b in zip(t1, t2))
        l1, l2 = mse_norm(dev, c["pred"], img, idx, p, 1.0, torch.float32), mse_norm(dev, c["pred"], img, idx, p, 1.0, torch.float32)
        assert torch.equal(l1[0], l2[0]) and torch.equal(l1[1], l2[1])
        r1, r2 = (restore_pixels(img.to(dev), c["pred"].to(dev), idx.to(dev), p) for _ in range(2))
        assert torch.equal(r1, r2)
        # alone = in the batch.  d_pred carries grad_scale * 2 / n: batch at grad_scale B and alone at 1 give the same real factor
        # (B * 2 / (B n1) = 2 / n1, both correctly rounded quotients of exact fp32 operands), so its rows compare bit for bit too
        dB = mse_norm(dev, c["pred"], img, idx, p, float(B), torch.float32)[1]
        for b in range(B):
            alone = gather_norm(dev, img[b:b + 1], idx[b:b + 1], p)
            assert all(torch.equal(a[0], full[b]) for a, full in zip(alone, t1)), (kind, b)
            assert torch.equal(restore_pixels(img[b:b + 1].to(dev), c["pred"][b:b + 1].to(dev), idx[b:b + 1].to(dev), p)[0], r1[b])
            assert torch.equal(mse_norm(dev, c["pred"][b:b + 1], img[b:b + 1], idx[b:b + 1], p, 1.0, torch.float32)[1][0], dB[b]), (kind, b)


@functools.lru_cache(maxsize=None)
def big_case(batch):
    """image 32, patch 4, m = 63 of the 64 patches: batch * 63 rows, the reference computed once."""
    S, p, C_, m = 32, 4, 3, 63
    g = torch.Generator().manual_seed(77 + batch)
    u8 = make_images(S, p, C_, batch, g)
    idx = torch.stack([torch.randperm(64, generator=g)[:m] + 1 for _ in range(batch)])
    t, _mean, rstd = NR.target_ref(u8, idx, p)
    pred = torch.randn(batch, m, p * p * C_, generator=g)
    loss, d = NR.loss_ref(pred, u8, idx, p)
    return dict(u8=u8, f32=NR.normalize_u8(u8), idx=idx, t=t, bound=NR.bound(t, rstd), pred=pred, loss=loss, d=d, x=NR.patches_ref(u8, idx, p))


@pytest.mark.parametrize("dt", ["u8", "f32"])
@pytest.mark.parametrize("batch", [130, 263])
def test_more_rows_than_the_grid_covers_at_once(dev, batch, dt):
    """A workgroup serves 4 rows per trip; the loss launches at most 1024 workgroups (its stage-1 partials), gather and restore at
    most 4096.  image 32, patch 4, m = 63: batch 130 gives 8190 rows = 2 trips of the loss (exactly 1024 partials, the last
    workgroup of the second trip with two of its four waves idle); batch 263 gives 16569 rows = 5 trips of the loss and 2 of
    gather and restore (one live wave in the last workgroup).  Every later trip reuses the waves' LDS slices."""
    p = 4
    c = big_case(batch)
    rows = batch * 63
    assert rows > 4 * 1024 and rows % 4 != 0 and (batch < 263 or rows > 4 * 4096)
    img, idx = c[dt], c["idx"]
    t, _m, _r = gather_norm(dev, img, idx, p)
    r = ratio(t, c["t"], c["bound"])
    loss, d = mse_norm(dev, c["pred"], img, idx, p, 1.0, torch.float32)
    rel = abs(loss.item() - c["loss"]) / c["loss"]
    rd = ratio(d, c["d"], c["bound"] * (2.0 / c["pred"].numel()) + 2.0 ** -22 * c["d"].abs())
    back = restore_pixels(img.to(dev), t, idx.to(dev), p)
    rb = ratio(back, c["x"], 2.0 ** -20 * (1 + c["x"].abs()))
    print(f"B={batch} {dt}: target max error / bound = {r:.4f}, loss rel err {rel:.3e}, d_pred max error / bound = {rd:.4f}, "
          f"restore max error / bound = {rb:.4f}")
    assert r <= 1.0 and rel <= 1e-5 and rd <= 1.0 and rb <= 1.0
    assert torch.equal(t[CONST], torch.zeros_like(t[CONST]))
    # a row of a later trip equals the same image served alone (first trip)
    last = batch - 1
    alone = gather_norm(dev, img[last:], idx[last:], p)[0]
    assert torch.equal(alone[0], t[last])


def test_patch_size_limit_is_the_same_for_the_three_calls(dev):
    """P = p*p*C <= 10236: four patches and the loss's reduction buffer share the LDS.  At the limit all three calls run; past it
    all three refuse before launching."""
    def run(C_, S):
        img = torch.rand(1, C_, S, S, generator=torch.Generator().manual_seed(1)) * 2 - 1
        idx = torch.ones(1, 1, dtype=torch.int64)
        P = S * S * C_
        pred = torch.zeros(1, 1, P, device=dev)
        out, loss, scratch = torch.empty(1, 1, P, device=dev), torch.empty(1, device=dev), torch.zeros(4096, device=dev)
        imgd, idxd = img.to(dev), idx.to(dev)
        rc = (lib.mae_patchify_gather_norm(_ptr(imgd), _lib.MAE_F32, _ptr(idxd), 1, C_, S, S, 1, _ptr(out), None, None, _stream(dev)),
              lib.mae_mse_loss_norm_pix(_ptr(pred), _ptr(imgd), _lib.MAE_F32, _ptr(idxd), 1, C_, S, S, 1, 1.0, _ptr(loss), None, _lib.MAE_F32,
                                        _ptr(scratch), _stream(dev)),
              lib.mae_norm_pix_restore(_ptr(imgd), _lib.MAE_F32, _ptr(pred), _ptr(idxd), 1, C_, S, S, 1, _ptr(pred), _stream(dev)))
        check(0)
        return rc, img, idx, out, loss
    rc, img, idx, out, loss = run(2559, 2)   # P = 10236
    assert rc == (0, 0, 0)
    t_ref, _mean, rstd_ref = NR.target_ref(img, idx, 2)
    assert ratio(out, t_ref, NR.bound(t_ref, rstd_ref)) <= 1.0
    assert abs(loss.item() - float((t_ref * t_ref).mean())) <= 1e-5 * float((t_ref * t_ref).mean())
    rc, *_ = run(2560, 2)                    # P = 10240
    assert all(v != 0 for v in rc), rc


def test_argument_checks(dev):
    img = torch.zeros(1, 3, 16, 16, device=dev)
    idx = torch.ones(1, 2, dtype=torch.int64, device=dev)
    out = torch.zeros(1, 2, 48, device=dev)
    for S, p in ((16, 5), (16, 0)):
        assert lib.mae_patchify_gather_norm(_ptr(img), _lib.MAE_F32, _ptr(idx), 1, 3, S, p, 2, _ptr(out), None, None, _stream(dev)) != 0
    assert lib.mae_patchify_gather_norm(_ptr(img), _lib.MAE_BF16, _ptr(idx), 1, 3, 16, 4, 2, _ptr(out), None, None, _stream(dev)) != 0
    assert lib.mae_patchify_gather_norm(_ptr(img), _lib.MAE_F32, _ptr(idx), 1, 3, 16, 4, 2, None, None, None, _stream(dev)) != 0
    big = torch.zeros(2, 2, 48, device=dev).view(-1)   # a partial overlap of pred and out is rejected
    assert lib.mae_norm_pix_restore(_ptr(img), _lib.MAE_F32, _ptr(big[:96]), _ptr(idx), 1, 3, 16, 4, 2, _ptr(big[48:144]), _stream(dev)) != 0
    check(0)
