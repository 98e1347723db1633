"""Normalised-pixel targets on the GPU (-m gpu), engine level: the fused step with ``norm_pix_loss`` against the autograd route
(whose backward is checked against the oracle by tests/test_gpu_engine.py) and against the float64 reference of
tests/normpix_ref.py, ``reconstruct()`` under the flag, and the two CLIs.

Tolerances: the project's fp32 ones (loss 1e-4 relative, per-tensor gradients 2e-4 relative) between the two routes; the kernel
bound of tests/normpix_ref.py for the target; 1e-5 relative for a loss against the float64 loss of the same prediction; the
per-image sums as in tests/test_gpu_reconstruction.py (gamma_n of an fp32 sum of n non-negative terms)."""
import json
import math

import pytest
import torch

from oracle import mae_oracle as O
from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
from ssrl_vit_mae_jepa_amd.mae import restore_pixels
from tests import normpix_ref as NR
from tests import recon_ref as R
from tests.test_gpu_engine import MICRO, cfg_dicts
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def build(cfg, precision, dev, flag=True, mask_ratio=0.75, seed=73):
    """tests.test_gpu_engine.build with the flag in the general config (flag None: the key is absent)."""
    params = O.init_params(cfg, seed)
    O.randomize_params(params)
    g, e, d = cfg_dicts(cfg, precision, mask_ratio)
    if flag is not None:
        g["norm_pix_loss"] = flag
    model = MaskedAutoencoder(g, e, d)
    model.load_state_dict(params, strict=True)
    return model.to(dev)


def make_images(cfg, B, u8: bool, seed=5):
    if not u8:
        return O.synthetic_images(B, cfg, seed=seed)
    return torch.randint(0, 256, (B, cfg.in_chans, cfg.image_size, cfg.image_size), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("cfg,B,r", [(MICRO, 3, 0.75), (O.YAML_TINY, 2, 0.5)], ids=["micro", "yaml_tiny"])
def test_fp32_fused_step_equals_autograd_route_and_fp64(dev, cfg, B, r, u8):
    model = build(cfg, "fp32", dev, mask_ratio=r)
    assert model.norm_pix_loss is True
    images = make_images(cfg, B, u8)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(74)).to(dev)
    loss_fused, keep, mask = model.loss_and_grads(images.to(dev), noise, return_indices=True)
    fused = {n: t.clone() for n, t in model.named_flat_views(model.flat_grads).items()}
    x_pred, target = model(images.to(dev), noise=noise)
    assert x_pred.requires_grad and not target.requires_grad
    loss = torch.nn.MSELoss()(x_pred, target)
    loss.backward()
    rel = abs(loss_fused.item() - loss.item()) / abs(loss.item())
    print(f"fused vs autograd loss rel err {rel:.3e}")
    assert rel <= 1e-4
    named = dict(model.named_parameters())
    for n, gf in fused.items():
        assert rel_err(gf, named[n].grad) < 2e-4, n
    # the autograd route's target is the standardised patch ...
    t_ref, _mean, rstd_ref = NR.target_ref(images, mask.cpu(), cfg.patch_size)
    ratio = float(((target.double().cpu() - t_ref).abs() / NR.bound(t_ref, rstd_ref)).max())
    print(f"target max error / bound = {ratio:.4f}")
    assert ratio <= 1.0
    # ... and both losses are the float64 loss of that prediction
    loss64, _d = NR.loss_ref(x_pred, images, mask.cpu(), cfg.patch_size)
    for got in (loss.item(), loss_fused.item()):
        assert abs(got - loss64) <= 1e-5 * loss64, (got, loss64)


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
def test_bf16_fused_loss_and_gradient_scaling(dev, u8):
    cfg, B = MICRO, 4
    model = build(cfg, "bf16", dev)
    images = make_images(cfg, B, u8).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(9)).to(dev)
    loss, _keep, mask = model.loss_and_grads(images, noise, return_indices=True)
    g1 = model.flat_grads.clone()
    with torch.no_grad():
        x_pred, _target = model(images, noise=noise)   # the same kernels on the same inputs: the step's x_pred
    loss64, _d = NR.loss_ref(x_pred, images.cpu(), mask.cpu(), cfg.patch_size)
    rel = abs(loss.item() - loss64) / loss64
    print(f"bf16 fused loss vs fp64 of its x_pred: rel err {rel:.3e}")
    assert rel <= 1e-5
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    loss_half = model.loss_and_grads(images, noise, grad_scale=0.5)
    g_half = model.flat_grads.clone()
    assert torch.equal(loss_half, loss)   # grad_scale scales the gradient, not the loss
    assert rel_err(g_half, 0.5 * g1) <= 2.0 ** -8


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_flag_changes_the_loss_and_off_is_the_default(dev, precision):
    cfg, B = MICRO, 3
    images = make_images(cfg, B, True).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(3)).to(dev)
    on, off, absent = (build(cfg, precision, dev, flag=f) for f in (True, False, None))
    assert (on.norm_pix_loss, off.norm_pix_loss, absent.norm_pix_loss) == (True, False, False)
    l_on, l_off, l_absent = (m.loss_and_grads(images, noise) for m in (on, off, absent))
    assert torch.equal(l_off, l_absent) and torch.equal(off.flat_grads, absent.flat_grads)
    assert l_on.item() != l_off.item() and not torch.equal(on.flat_grads, off.flat_grads)
    assert torch.equal(off.patchify_gather(images, on.random_token_mask(B, noise)[1]), absent.patchify_gather(images, on.random_token_mask(B, noise)[1]))
    # patchify_gather follows the flag unless told otherwise
    mask = on.random_token_mask(B, noise)[1]
    assert torch.equal(on.patchify_gather(images, mask, normalize=False), off.patchify_gather(images, mask))
    assert torch.equal(off.patchify_gather(images, mask, normalize=True), on.patchify_gather(images, mask))


@pytest.mark.parametrize("u8", [False, True], ids=["f32img", "u8img"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_reconstruct_under_the_flag(dev, precision, u8):
    cfg, B = MICRO, 3
    model = build(cfg, precision, dev)
    images = make_images(cfg, B, u8, seed=11)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(21)).to(dev)
    r = model.reconstruct(images.to(dev), noise=noise)
    with torch.no_grad():
        x_dec = model.forward_decoder(model.forward_encoder(images.to(dev), r.idx_keep), r.idx_keep, r.idx_mask)
    assert torch.equal(r.x_pred, x_dec)   # normalised space: what forward_decoder returns
    restored = model.restore_pixels(images.to(dev), r.x_pred, r.idx_mask)
    assert torch.equal(restored, restore_pixels(images.to(dev), r.x_pred, r.idx_mask, cfg.patch_size))
    want, _masked = R.compose_ref(images, restored, r.idx_mask, cfg.patch_size)
    assert torch.equal(r.reconstructed.cpu(), want)   # masked patches = the restored prediction, visible pixels = the input, bit for bit
    x = R.normalize_u8(images)
    patches = O.patchify(x, cfg.patch_size)
    vis = torch.ones(B, patches.shape[1], dtype=torch.bool)
    vis.scatter_(1, r.idx_mask.cpu() - 1, False)
    assert torch.equal(O.patchify(r.reconstructed.cpu(), cfg.patch_size)[vis], patches[vis]) and vis.any()
    sq, ab = R.sums_ref(images, r.reconstructed)
    n = r.idx_mask.shape[1] * cfg.patch_size ** 2 * cfg.in_chans + 2
    bound = R.gamma(n)
    assert n <= 3074 and bound < 1.9e-4
    for got, ref in ((r.sum_sq, sq), (r.sum_abs, ab)):
        err = (got.double().cpu() - ref).abs() / ref
        print("sum rel err", err.tolist(), "bound", bound)
        assert (err <= bound).all()
    # the same model without the flag reads the prediction as pixels: another image
    assert not torch.equal(build(cfg, precision, dev, flag=False).reconstruct(images.to(dev), noise=noise).reconstructed, r.reconstructed)


def test_clis_carry_the_flag(dev, tmp_path, monkeypatch, capsys):
    import yaml
    from pathlib import Path
    from scripts.evaluation import visualize_reconstruction as V
    from scripts.training import pretrain_mae
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load(open(root / "configs" / "mae.yaml"))
    assert "norm_pix_loss" not in cfg["model"]["general"]
    cfg["pretrain"].update(batch_size=16, total_epochs=1, warmup_epochs=1)   # 64 synthetic images -> three fused steps and a validation batch
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg_path = tmp_path / "mae.yaml"
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    monkeypatch.chdir(tmp_path)
    pretrain_mae.main(["--config", str(cfg_path), "--output_dir_suffix", "np", "--synthetic_images", "64", "--max_epochs", "1", "--norm_pix_loss"])
    out = tmp_path / "outputs" / "pretrain" / "np"
    rec = json.loads((out / "logs" / "metrics.jsonl").read_text().strip().splitlines()[-1])
    assert rec["norm_pix_loss"] is True and math.isfinite(rec["train_loss"]) and math.isfinite(rec["val_loss"])
    ck = torch.load(out / "checkpoints" / "last.ckpt", weights_only=True)
    assert ck["hyper_parameters"]["model_cfg"]["general"]["norm_pix_loss"] is True and ck["global_step"] >= 3
    assert yaml.safe_load(open(out / "config.yaml"))["model"]["general"]["norm_pix_loss"] is True
    # the checkpoint says what it was trained with: no flag on the command line, a config that does not mention it
    capsys.readouterr()
    res = V.main(["--config", str(cfg_path), "--model_path", str(out / "checkpoints" / "last.ckpt"), "--synthetic_images", "16", "--num_samples", "3",
                  "--output_dir", str(tmp_path / "viz")])
    assert res["norm_pix_loss"] is True and res["layout"] == "state_dict" and "taken from the checkpoint" in capsys.readouterr().out
    assert all(math.isfinite(res["sample"][k]) for k in ("mse", "l1", "psnr", "masked_mse"))
    # the bare state dict needs the flag
    raw = V.main(["--config", str(cfg_path), "--model_path", str(out / "vit-mae.pt"), "--synthetic_images", "16", "--num_samples", "3",
                  "--output_dir", str(tmp_path / "viz_raw"), "--norm_pix_loss"])
    assert raw["norm_pix_loss"] is True and raw["layout"] == "raw" and raw["sample"] == res["sample"]
