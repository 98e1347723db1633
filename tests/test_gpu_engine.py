"""Engine-level parity (-m gpu): MaskedAutoencoder over libmae_hip.so against the CPU oracle on identical seeded
weights / images / noise.  PARITY UNPINNED w.r.t. lightly/timm themselves (see oracle/mae_oracle.py header): the oracle
is our restatement, pinned only by the reference's structure known-answers.

Tolerances (north_star): mask indices bit-exact; fp32 engine loss within 1e-4 relative of the fp32 oracle; the bf16
engine is compared with the oracle's bf16-operand emulation (loss 5e-3 relative) and with the fp32 oracle (3e-2)."""
import copy
import json

import pytest
import torch

from oracle import mae_oracle as O
from ssrl_vit_mae_jepa_amd import MAEPretrainModule, MaskedAutoencoder
from tests.util import rel_err

pytestmark = pytest.mark.gpu

MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


def cfg_dicts(cfg: O.MAEConfig, precision: str, mask_ratio=0.75):
    return (dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, mask_ratio=mask_ratio,
                 engine_precision=precision),
            dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
            dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth,
                 decoder_num_heads=cfg.decoder_num_heads))


def build(cfg, precision, dev, mask_ratio=0.75, seed=73):
    params = O.init_params(cfg, seed)
    O.randomize_params(params)
    model = MaskedAutoencoder(*cfg_dicts(cfg, precision, mask_ratio))
    model.load_state_dict(params, strict=True)
    return model.to(dev), params


CASES = [(MICRO, 2, 0.75), (MICRO, 5, 0.5), (O.YAML_TINY, 2, 0.75), (O.YAML_TINY, 5, 0.5)]


@pytest.mark.parametrize("cfg,B,r", CASES)
def test_fp32_forward_and_grads_match_oracle(dev, cfg, B, r):
    model, params = build(cfg, "fp32", dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(74))
    loss_ref, grads_ref, aux = O.loss_and_grads(params, cfg, images, noise, r)
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    for n, gr in grads_ref.items():
        assert rel_err(g[n], gr) < 2e-4, n
    # API pieces: forward_encoder / forward_decoder / target
    x_enc = model.forward_encoder(images.to(dev), keep)
    assert rel_err(x_enc, aux["x_encoded"]) < 1e-4
    x_pred = model.forward_decoder(x_enc, keep, mask)
    assert rel_err(x_pred, aux["x_pred"]) < 1e-4
    assert torch.equal(model.patchify_gather(images.to(dev), mask).cpu(), aux["target"])


@pytest.mark.parametrize("cfg,B,r", CASES)
def test_bf16_engine_close_to_bf16_emulating_oracle(dev, cfg, B, r):
    model, params = build(cfg, "bf16", dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(74))
    loss_emu, grads_emu, aux = O.loss_and_grads(params, cfg, images, noise, r, bf16=True)
    loss_f32, _, _ = O.loss_and_grads(params, cfg, images, noise, r)
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_emu.item()) <= 5e-3 * abs(loss_emu.item())
    assert abs(loss.item() - loss_f32.item()) <= 3e-2 * abs(loss_f32.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_emu.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_emu.values())
    assert (num / den) ** 0.5 < 5e-2


@pytest.mark.parametrize("precision,tol", [("fp32", 2e-5), ("bf16", 2e-2)])
def test_two_fused_steps_match_oracle(dev, precision, tol):
    cfg, B = MICRO, 4
    tcfg = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=800, warmup_epochs=20,
                batch_size=2000, base_learning_rate=1.5e-4, weight_decay=0.05)
    g, e, d = cfg_dicts(cfg, precision)
    module = MAEPretrainModule(dict(general=g, encoder=e, decoder=d), tcfg)
    params = O.init_params(cfg, 73); O.randomize_params(params)
    module.model.load_state_dict(params)
    module = module.to(dev)
    module.on_train_epoch_start()
    lr = O.effective_lr(1.5e-4, 2000) * O.lr_lambda(0, 20, 800)
    assert abs(module.current_lr() - lr) < 1e-12 and abs(lr - 1.171875e-3 * 0.05) < 1e-12
    state = {}
    for step in (1, 2):
        images = O.synthetic_images(B, cfg, seed=100 + step)
        noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(73 + step))
        loss_ref, aux = O.train_step(params, cfg, state, images, noise, lr, step, bf16=(precision == "bf16"))
        loss = module.fused_training_step(images.to(dev), noise.to(dev))
        assert abs(loss.item() - loss_ref.item()) <= (1e-4 if precision == "fp32" else 5e-3) * abs(loss_ref.item())
        stats = module._stats.cpu()
        assert abs(stats[0].item() - float(aux["grad_norm"])) <= (2e-4 if precision == "fp32" else 5e-2) * float(aux["grad_norm"])
    sd = module.model.state_dict()
    for n in O.trainable_names(cfg):
        assert rel_err(sd[n], params[n]) < tol, n
    for n in O.FROZEN + O.NO_GRAD_ON_PATH:  # never touched by clip/AdamW (grad None in the reference)
        assert torch.equal(sd[n].cpu(), params[n])


def test_twelve_fused_steps_track_the_oracle(dev):
    """A longer trajectory than the two-step check: twelve whole steps (fresh images and masks each step, warm-up learning
    rate, clip active at first) in the fp32 engine against oracle.train_step; the loss of every step within 2e-4 relative, the
    parameters after the last step within 2e-4 -- rounding differences must not compound."""
    cfg, B = MICRO, 6
    tcfg = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=800, warmup_epochs=20,
                batch_size=2000, base_learning_rate=1.5e-4, weight_decay=0.05)
    g, e, d = cfg_dicts(cfg, "fp32")
    module = MAEPretrainModule(dict(general=g, encoder=e, decoder=d), tcfg)
    params = O.init_params(cfg, 73); O.randomize_params(params)
    module.model.load_state_dict(params)
    module = module.to(dev)
    module.on_train_epoch_start()
    lr = O.effective_lr(1.5e-4, 2000) * O.lr_lambda(0, 20, 800)
    state, losses = {}, []
    for step in range(1, 13):
        images = O.synthetic_images(B, cfg, seed=300 + step)
        noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(500 + step))
        loss_ref, _aux = O.train_step(params, cfg, state, images, noise, lr, step)
        loss = module.fused_training_step(images.to(dev), noise.to(dev))
        losses.append((loss.item(), loss_ref.item()))
    for got, ref in losses:
        assert abs(got - ref) <= 2e-4 * abs(ref), losses
    sd = module.model.state_dict()
    for n in O.trainable_names(cfg):
        assert rel_err(sd[n], params[n]) < 2e-4, n


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_autograd_path_equals_fused_path(dev, precision):
    cfg, B = MICRO, 3
    model, _ = build(cfg, precision, dev)
    images = O.synthetic_images(B, cfg).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(1)).to(dev)
    loss_fused = model.loss_and_grads(images, noise)
    fused = {n: t.clone() for n, t in model.named_flat_views(model.flat_grads).items()}
    preds, targets = model(images, noise=noise)
    assert preds.requires_grad and not targets.requires_grad
    loss = torch.nn.MSELoss()(preds, targets)
    loss.backward()
    assert abs(loss.item() - loss_fused.item()) < 1e-5 * abs(loss.item())
    named = dict(model.named_parameters())
    for n, gf in fused.items():
        tol = 1e-5 if precision == "fp32" else 1e-2  # d_pred is rounded to bf16 at different points
        assert rel_err(named[n].grad, gf) < tol, n
    for n in O.FROZEN + O.NO_GRAD_ON_PATH:
        assert named[n].grad is None


def test_external_optimizer_refreshes_operand_copies(dev):
    cfg, B = MICRO, 3
    model, _ = build(cfg, "bf16", dev)
    images = O.synthetic_images(B, cfg).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(1)).to(dev)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2, weight_decay=0.05)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        p, t = model(images, noise=noise)
        loss = torch.nn.functional.mse_loss(p, t)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)
        opt.step()
        losses.append(loss.item())
    assert losses[2] < losses[0]  # the engine sees the updated weights (bf16 copies were refreshed)


def test_error_behaviour(dev):
    model, _ = build(MICRO, "fp32", dev)
    with pytest.raises(ValueError):
        model(torch.zeros(2, 3, 40, 40, device=dev))  # timm PatchEmbed asserts the image size
    with pytest.raises(IndexError):
        model.forward_encoder(torch.zeros(1, 3, 32, 32, device=dev), torch.tensor([[0, 99]], device=dev))
    with pytest.raises(ValueError):
        MaskedAutoencoder(dict(image_size=32, patch_size=8), dict(embed_dim=50, depth=1, num_heads=4),
                          dict(decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2))


def test_forward_features_all_tokens(dev):
    cfg = MICRO
    model, params = build(cfg, "fp32", dev)
    images = O.synthetic_images(2, cfg)
    ref = O.forward_encoder(params, cfg, images, None)
    out = model.encoder.vit.forward_features(images.to(dev))
    assert out.shape == (2, cfg.sequence_length, cfg.embed_dim) and rel_err(out, ref) < 1e-4


# ------------------------------------------------------------------------------------------------------------------
# full BASELINE size (ViT-S/8 96px, B=2000): size-independent properties (the oracle would take minutes here)
# ------------------------------------------------------------------------------------------------------------------
def _full_size_properties(dev, cfg, B):
    model = MaskedAutoencoder(*cfg_dicts(cfg, "bf16")).to(dev)
    g = torch.Generator(device=dev).manual_seed(73)
    images = torch.rand(B, cfg.in_chans, cfg.image_size, cfg.image_size, device=dev, generator=g) * 2 - 1
    noise = torch.rand(B, cfg.sequence_length, device=dev, generator=g)
    loss1, keep, mask = model.loss_and_grads(images, noise, return_indices=True)
    g1 = model.flat_grads.clone()
    # (1) keep U mask is a permutation of the tokens, class token first, noise ascending
    allidx = torch.cat([keep, mask], 1)
    assert keep.shape[1] == cfg.num_keep()
    assert torch.equal(allidx.sort(1).values, torch.arange(cfg.sequence_length, device=dev).repeat(B, 1))
    assert bool((keep[:, 0] == 0).all())
    nz = noise.clone(); nz[:, 0] = -1
    assert bool((torch.gather(nz, 1, allidx).diff(dim=1) >= 0).all())
    # (2) finite, sane loss for random-init weights on U[-1,1] pixels
    assert torch.isfinite(loss1).all() and 0.05 < loss1.item() < 5.0
    assert torch.isfinite(g1).all() and g1.norm().item() > 0
    # (3) linearity in the loss-gradient scale (data-parallel 1/world factor)
    loss2 = model.loss_and_grads(images, noise, grad_scale=0.5)
    assert abs(loss2.item() - loss1.item()) <= 1e-5 * abs(loss1.item())
    assert rel_err(model.flat_grads, 0.5 * g1) < 2e-2
    # (4) batch-shard consistency: mean of two half-batch gradients == full-batch gradient (what DP all-reduce relies on)
    h = B // 2
    model.loss_and_grads(images[:h].contiguous(), noise[:h].contiguous(), grad_scale=0.5)
    ga = model.flat_grads.clone()
    model.loss_and_grads(images[h:].contiguous(), noise[h:].contiguous(), grad_scale=0.5)
    assert rel_err(ga + model.flat_grads, g1) < 2e-2
    # (5) frozen position tables and the unreachable encoder mask token are outside the optimizer range
    assert model.engine.trainable_elems < model.engine.arena_elems
    assert model.engine.trainable_elems >= sum(torch.Size(s).numel() for n, s in O.param_shapes(cfg).items() if n in O.trainable_names(cfg))


def test_full_size_properties_vits8_b2000(dev):
    _full_size_properties(dev, O.VIT_S8_YAMLDEC, 2000)


def test_full_size_properties_vitb16_b512(dev):
    """BASELINE.json configs[3] at its per-GPU batch (global 4096 over 8 GPUs): K = 768 / 3072, N = 2304 GEMMs, 49- and
    197-token attention (head dims 64 and 32), 512-wide decoder on the 128 x 128 wgrad tiles."""
    _full_size_properties(dev, O.VIT_B16_DEC512, 512)


# ------------------------------------------------------------------------------------------------------------------
# committed golden vectors (tests/golden/mae_micro.npz) and the caller of the path (pretrain CLI)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,r", [("b2_r75", 0.75), ("b5_r50", 0.5)])
def test_fp32_engine_matches_committed_golden(dev, tag, r):
    import numpy as np
    from pathlib import Path
    gold = np.load(Path(__file__).parent / "golden" / "mae_micro.npz")
    T = lambda k: torch.from_numpy(gold[f"{tag}/{k}"])  # noqa: E731
    model, params = build(MICRO, "fp32", dev, r)
    loss, keep, mask = model.loss_and_grads(T("images").to(dev), T("noise").to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), T("idx_keep")) and torch.equal(mask.cpu(), T("idx_mask"))
    assert abs(loss.item() - float(T("loss"))) <= 1e-4 * float(T("loss"))
    g = model.named_flat_views(model.flat_grads)
    names = O.trainable_names(MICRO)
    assert rel_err(torch.stack([g[n].norm() for n in names]), T("grad_norms")) < 2e-4
    for k in gold.files:
        if k.startswith(f"{tag}/grad/"):
            assert rel_err(g[k.split("/", 2)[2]], torch.from_numpy(gold[k])) < 2e-4, k
    assert torch.equal(model.patchify_gather(T("images").to(dev), mask).cpu(), T("target"))
    # tie case: equal keys ordered by index
    noise, stable = torch.from_numpy(gold["ties/noise"]), torch.from_numpy(gold["ties/order_stable"])
    m17 = MaskedAutoencoder(dict(image_size=32, patch_size=8, mask_ratio=0.75, engine_precision="fp32"),
                            dict(embed_dim=48, depth=1, num_heads=2), dict(decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)).to(dev)
    k2, m2 = m17.random_token_mask(3, noise.to(dev))
    assert torch.equal(torch.cat([k2, m2], 1).cpu(), stable)


def test_pretrain_cli_synthetic_run_and_resume(dev, tmp_path, monkeypatch):
    import yaml
    from pathlib import Path
    from scripts.training import pretrain_mae as cli
    cfg = yaml.safe_load(open(Path(__file__).resolve().parents[1] / "configs" / "mae.yaml"))
    cfg["pretrain"].update(batch_size=32, total_epochs=3, warmup_epochs=2)
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg_path = tmp_path / "mae.yaml"
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    monkeypatch.chdir(tmp_path)
    cli.main(["--config", str(cfg_path), "--output_dir_suffix", "t", "--synthetic_images", "128", "--max_epochs", "2"])
    out = tmp_path / "outputs" / "pretrain" / "t"
    assert (out / "config.yaml").exists() and (out / "vit-mae.pt").exists()
    assert (out / "checkpoints" / "last.ckpt").exists() and (out / "checkpoints" / "best.ckpt").exists()
    ck = torch.load(out / "checkpoints" / "last.ckpt", weights_only=True)
    assert ck["epoch"] == 1 and all(k.startswith("model.") for k in ck["state_dict"])
    assert "model.encoder.vit.blocks.0.attn.qkv.weight" in ck["state_dict"]
    opt = ck["optimizer_states"][0]  # torch.optim.AdamW.state_dict() layout, indexed in parameters() order
    assert opt["param_groups"][0]["params"] == list(range(len(ck["state_dict"])))
    assert all(float(st["step"]) == ck["global_step"] for st in opt["state"].values()) and 0 not in opt["state"]  # index 0 = encoder.mask_token: no grad
    assert ck["hyper_parameters"]["training_cfg"]["batch_size"] == 32 and ck["lr_schedulers"][0]["last_epoch"] == 2
    assert ck["best_val_loss"] <= ck["val_loss"]
    raw = torch.load(out / "vit-mae.pt", weights_only=True)
    assert list(raw) == list(O.param_shapes(O.YAML_TINY))  # raw state_dict, reference key names
    lines = (out / "logs" / "metrics.jsonl").read_text().strip().splitlines()
    assert len(lines) == 2
    cli.main(["--config", str(cfg_path), "--output_dir_suffix", "t", "--synthetic_images", "128",
              "--resume_from", str(out / "checkpoints" / "last.ckpt")])
    ck2 = torch.load(out / "checkpoints" / "last.ckpt", weights_only=True)
    assert ck2["epoch"] == 2 and ck2["global_step"] > ck["global_step"]
    assert ck2["best_val_loss"] <= ck["best_val_loss"]  # the best validation loss survives the resume
    recs = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().strip().splitlines()]
    assert len(recs) == 3 and 0.0 < recs[2]["train_loss"] < 2 * recs[0]["train_loss"]  # per-epoch mean, not divided by all steps since the start


# ------------------------------------------------------------------------------------------------------------------
# ViT-S/8 geometry (the MFMA kernels' shapes) at other mask ratios: k = 72 / 36 / 21 visible tokens
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,B", [(0.5, 6), (0.75, 7), (0.86, 9)])
def test_vits8_bf16_matches_emulating_oracle_at_other_mask_ratios(dev, r, B):
    cfg = O.VIT_S8_YAMLDEC
    model, params = build(cfg, "bf16", dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(5))
    loss_emu, grads_emu, aux = O.loss_and_grads(params, cfg, images, noise, r, bf16=True)
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert keep.shape[1] == cfg.num_keep(r) and torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_emu.item()) <= 5e-3 * abs(loss_emu.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_emu.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_emu.values())
    assert (num / den) ** 0.5 < 5e-2


def test_vits8_fp32_matches_oracle(dev):
    cfg, B, r = O.VIT_S8_YAMLDEC, 3, 0.75
    model, params = build(cfg, "fp32", dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(5))
    loss_ref, grads_ref, aux = O.loss_and_grads(params, cfg, images, noise, r)
    loss = model.loss_and_grads(images.to(dev), noise.to(dev))
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_ref.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_ref.values())
    assert (num / den) ** 0.5 < 2e-4


# the code-default decoder (512 wide, 4 deep) with 8 heads: head dim 64, 145 tokens -> the
# 5-chunk attention kernels, K = 512 / 2048 GEMMs, 192-multiple wgrad tiles not available (512 % 192 != 0)
@pytest.mark.parametrize("prec,B,tol_loss,tol_grad", [("bf16", 3, 5e-3, 5e-2), ("fp32", 2, 1e-4, 2e-4)])
def test_vits8_dec512_matches_oracle(dev, prec, B, tol_loss, tol_grad):
    cfg, r = O.VIT_S8_DEC512, 0.75
    model, params = build(cfg, prec, dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(9))
    loss_ref, grads_ref, aux = O.loss_and_grads(params, cfg, images, noise, r, bf16=(prec == "bf16"))
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_ref.item()) <= tol_loss * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_ref.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_ref.values())
    assert (num / den) ** 0.5 < tol_grad


# BASELINE.json configs[3]: ViT-B/16 224 px + decoder 512 x 8 x 16 heads (k = 49, m = 148, L = 197, P = 768)
@pytest.mark.parametrize("prec,B,tol_loss,tol_grad", [("fp32", 2, 1e-4, 2e-4), ("bf16", 3, 5e-3, 5e-2)])
def test_vitb16_matches_oracle(dev, prec, B, tol_loss, tol_grad):
    cfg, r = O.VIT_B16_DEC512, 0.75
    assert (cfg.sequence_length, cfg.num_keep(r), cfg.patch_dim) == (197, 49, 768)
    assert abs(O.flops_per_image_step(cfg) / 1e9 - 57.5245) < 1e-3
    model, params = build(cfg, prec, dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(13))
    loss_ref, grads_ref, aux = O.loss_and_grads(params, cfg, images, noise, r, bf16=(prec == "bf16"))
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_ref.item()) <= tol_loss * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_ref.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_ref.values())
    assert (num / den) ** 0.5 < tol_grad
    if prec == "fp32":
        for n, gr in grads_ref.items():
            assert rel_err(g[n], gr) < 5e-4, n
        x_enc = model.forward_encoder(images.to(dev), keep)
        assert rel_err(x_enc, aux["x_encoded"]) < 1e-4
        assert rel_err(model.forward_decoder(x_enc, keep, mask), aux["x_pred"]) < 1e-4


# Other geometries than the reference's 96 px / patch 8 / 3 channels: the kernels are not specialised to them
GEOMS = [
    (O.MAEConfig(image_size=64, patch_size=16, in_chans=3, embed_dim=192, depth=2, num_heads=3, decoder_embed_dim=128, decoder_depth=1, decoder_num_heads=4), 4, 0.6),
    (O.MAEConfig(image_size=48, patch_size=4, in_chans=1, embed_dim=64, depth=1, num_heads=2, decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2), 3, 0.8),
    (O.MAEConfig(image_size=112, patch_size=16, in_chans=3, embed_dim=384, depth=1, num_heads=6, decoder_embed_dim=192, decoder_depth=1, decoder_num_heads=6), 9, 0.75),
]


@pytest.mark.parametrize("cfg,B,r", GEOMS)
@pytest.mark.parametrize("prec,tol_loss,tol_grad", [("fp32", 1e-4, 3e-4), ("bf16", 5e-3, 5e-2)])
def test_other_geometries_match_oracle(dev, cfg, B, r, prec, tol_loss, tol_grad):
    model, params = build(cfg, prec, dev, r)
    images = O.synthetic_images(B, cfg)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(11))
    loss_ref, grads_ref, aux = O.loss_and_grads(params, cfg, images, noise, r, bf16=(prec == "bf16"))
    loss, keep, mask = model.loss_and_grads(images.to(dev), noise.to(dev), return_indices=True)
    assert torch.equal(keep.cpu(), aux["idx_keep"]) and torch.equal(mask.cpu(), aux["idx_mask"])
    assert abs(loss.item() - loss_ref.item()) <= tol_loss * abs(loss_ref.item())
    g = model.named_flat_views(model.flat_grads)
    num = sum(float((g[n].double().cpu() - gr.double()).pow(2).sum()) for n, gr in grads_ref.items())
    den = sum(float(gr.double().pow(2).sum()) for gr in grads_ref.values())
    assert (num / den) ** 0.5 < tol_grad


@pytest.mark.parametrize("B", [1, 7, 129, 1001])
def test_vits8_bf16_tracks_fp32_engine_over_batch_sizes(dev, B):
    """Ragged row counts through every kernel (M = 36 B and 145 B rows: partial GEMM tiles, partial wgrad steps, one
    workgroup per (image, head)): the bf16 path stays within bf16 noise of the exact-fp32 path of the same engine."""
    cfg = O.VIT_S8_YAMLDEC
    out = {}
    g = torch.Generator(device=dev).manual_seed(B)
    images = torch.rand(B, 3, 96, 96, device=dev, generator=g) * 2 - 1
    noise = torch.rand(B, cfg.sequence_length, device=dev, generator=g)
    for prec in ("fp32", "bf16"):
        torch.manual_seed(3)
        model = MaskedAutoencoder(*cfg_dicts(cfg, prec)).to(dev)
        loss = model.loss_and_grads(images, noise)
        torch.cuda.synchronize()
        assert torch.isfinite(model.flat_grads).all()
        out[prec] = (float(loss), model.flat_grads.clone())
    assert abs(out["bf16"][0] - out["fp32"][0]) <= 1e-3 * abs(out["fp32"][0])
    assert float((out["bf16"][1] - out["fp32"][1]).norm() / out["fp32"][1].norm()) < 5e-2


def test_step_is_hip_graph_capturable(dev):
    """The engine only enqueues on the caller's stream (no allocation, no sync): after one eager call (lazy attribute
    setup) a whole step can be captured into a graph and replayed with the same bits."""
    cfg, B = MICRO, 4
    g, e, d = cfg_dicts(cfg, "bf16")
    tcfg = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=800, warmup_epochs=20,
                batch_size=2000, base_learning_rate=1.5e-4, weight_decay=0.05)
    torch.manual_seed(0)
    module = MAEPretrainModule(dict(general=g, encoder=e, decoder=d), tcfg).to(dev)
    images = O.synthetic_images(B, cfg).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(1)).to(dev)
    model = module.model
    eager = model.loss_and_grads(images, noise).clone()   # warm-up: workspace, weight cache, function attributes
    grads_eager = model.flat_grads.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(stream):
        model.loss_and_grads(images, noise)  # once more on the capture stream before capturing
        with torch.cuda.graph(graph, stream=stream):
            loss_static = model.loss_and_grads(images, noise)
    model.flat_grads.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(loss_static, eager) and torch.equal(model.flat_grads, grads_eager)


# ------------------------------------------------------------------------------------------------------------------
# boundary pieces the reference's other callers touch: the classifier hand-off and the decoder's methods
# ------------------------------------------------------------------------------------------------------------------
def _grads_vs_oracle(named, grads_ref, tol):
    num = sum(float((named[n].grad.double().cpu() - g.double()).pow(2).sum()) for n, g in grads_ref.items())
    den = sum(float(g.double().pow(2).sum()) for g in grads_ref.values())
    assert (num / den) ** 0.5 < tol


@pytest.mark.parametrize("prec,tol", [("fp32", 2e-4), ("bf16", 5e-2)])
def test_finetune_head_on_forward_features_has_oracle_encoder_grads(dev, prec, tol):
    """scripts/training/train_mae.py:143 hands mae.encoder.vit to ViTClassifier (src/models/classifier.py:47-57):
    feats = encoder.forward_features(x); pooled = feats[:, 0]; logits = head(pooled); loss.backward() must reach the
    encoder's weights."""
    cfg, B = MICRO, 6
    model, params = build(cfg, prec, dev)
    vit = model.encoder.vit
    images = O.synthetic_images(B, cfg)
    labels = torch.arange(B) % 3
    torch.manual_seed(0)
    head = torch.nn.Linear(cfg.embed_dim, 3)
    # oracle: the same classifier over the CPU restatement of forward_features
    enc_names = [n for n in O.trainable_names(cfg) if n.startswith("encoder.")]
    leaves = {n: (params[n].clone().requires_grad_(True) if n in enc_names else params[n]) for n in params}
    feats_ref = O.forward_encoder(leaves, cfg, images, None, bf16=(prec == "bf16"))
    loss_ref = torch.nn.functional.cross_entropy(head(feats_ref[:, 0]), labels)
    grads_ref = dict(zip(enc_names, torch.autograd.grad(loss_ref, [leaves[n] for n in enc_names])))
    # engine
    head_d = copy.deepcopy(head).to(dev)
    feats = vit.forward_features(images.to(dev))
    assert feats.requires_grad and feats.shape == (B, cfg.sequence_length, cfg.embed_dim)
    loss = torch.nn.functional.cross_entropy(head_d(feats[:, 0]), labels.to(dev))
    loss.backward()
    assert abs(loss.item() - loss_ref.item()) <= (1e-4 if prec == "fp32" else 2e-2) * abs(loss_ref.item())
    named = dict(model.named_parameters())
    _grads_vs_oracle(named, grads_ref, tol)
    assert all(named[n].grad is None for n in named if n.startswith("decoder.")) and head_d.weight.grad is not None
    # a few steps of an ordinary optimizer over head + encoder lower the loss (the engine sees the updated weights)
    opt = torch.optim.AdamW(list(head_d.parameters()) + list(vit.parameters()), lr=2e-3)
    first = last = None
    for _ in range(8):
        opt.zero_grad(set_to_none=True)
        last = torch.nn.functional.cross_entropy(head_d(vit.forward_features(images.to(dev))[:, 0]), labels.to(dev))
        last.backward()
        opt.step()
        first = first if first is not None else last.item()
    assert last.item() < first


def test_encoder_blocks_are_indexable_like_timm(dev):
    """src/training/classifier.py:144-165 (unfreeze_last_layers): len(blocks), blocks[total-n:], block.parameters(), norm."""
    cfg = MICRO
    model, params = build(cfg, "fp32", dev)
    enc = model.encoder.vit
    blocks = enc.blocks
    assert len(blocks) == cfg.depth and len(model.decoder.decoder_blocks) == cfg.decoder_depth
    for p in enc.parameters():
        p.requires_grad = False
    for block in blocks[len(blocks) - 1:]:
        for p in block.parameters():
            p.requires_grad = True
    for p in enc.norm.parameters():
        p.requires_grad = True
    assert sum(p.numel() for p in blocks[0].parameters()) == sum(p.numel() for p in blocks[-1].parameters()) > 0
    images = O.synthetic_images(3, cfg)
    enc.forward_features(images.to(dev))[:, 0].square().mean().backward()
    named = dict(model.named_parameters())
    last = f"encoder.vit.blocks.{cfg.depth - 1}."
    assert named[last + "mlp.fc1.weight"].grad is not None and named["encoder.vit.norm.weight"].grad is not None
    assert named["encoder.vit.blocks.0.mlp.fc1.weight"].grad is None and named["encoder.vit.patch_embed.proj.weight"].grad is None
    # the partially frozen gradients are the oracle's
    leaves = {n: (t.clone().requires_grad_(True) if (n.startswith(last) or n.startswith("encoder.vit.norm.")) else t) for n, t in params.items()}
    ref = O.forward_encoder(leaves, cfg, images, None)[:, 0].square().mean()
    want = [n for n in leaves if leaves[n].requires_grad]
    for n, g in zip(want, torch.autograd.grad(ref, [leaves[n] for n in want])):
        assert rel_err(named[n].grad, g) < 2e-4, n


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("bf16", 2e-2)])
def test_two_node_path_equals_fused_node_and_extra_gradient(dev, prec, tol):
    """forward_encoder -> forward_decoder as separate autograd nodes == the single-node forward(); a second consumer of
    x_encoded adds its gradient at the encoder output (the d_x_encoded_extra argument of mae_engine_backward)."""
    import ctypes as C
    from ssrl_vit_mae_jepa_amd._lib import check, lib, ptr
    cfg, B = MICRO, 4
    model, _ = build(cfg, prec, dev)
    images = O.synthetic_images(B, cfg).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(2)).to(dev)
    keep, mask = model.random_token_mask(B, noise)
    probe = torch.randn(B, keep.shape[1], cfg.embed_dim, generator=torch.Generator().manual_seed(3)).to(dev) * 0.1
    named = dict(model.named_parameters())

    def collect():
        out = {n: p.grad.clone() for n, p in named.items() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        return out

    preds, targets = model(images, noise=noise)
    torch.nn.functional.mse_loss(preds, targets).backward()
    fused = collect()
    x_enc = model.forward_encoder(images, keep)
    x_pred = model.forward_decoder(x_enc, keep, mask)
    assert x_enc.requires_grad and x_pred.requires_grad and rel_err(x_pred, preds) < tol
    torch.nn.functional.mse_loss(x_pred, model.patchify_gather(images, mask)).backward()
    split = collect()
    assert set(split) == set(fused)
    for n in fused:
        assert rel_err(split[n], fused[n]) < tol, n
    # extra consumer of x_encoded: loss + <probe, x_encoded>
    x_enc = model.forward_encoder(images, keep)
    x_pred = model.forward_decoder(x_enc, keep, mask)
    (torch.nn.functional.mse_loss(x_pred, targets) + (x_enc * probe).sum()).backward()
    both = collect()
    preds2, _ = model._run_forward(images, keep, mask)
    d_pred = (2.0 / preds2.numel()) * (preds2 - targets)
    ws = model._ws(B, keep.shape[1], keep=True)
    g = torch.zeros(model.engine.trainable_elems, device=dev)
    check(lib.mae_engine_backward(model.engine.handle, ptr(model.flat_params), ptr(model._weights()), ptr(d_pred.contiguous()), ptr(probe.contiguous()),
                                 B, keep.shape[1], mask.shape[1], ptr(ws), ws.numel(), ptr(g), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    direct = model.named_flat_views(g)
    for n in both:
        assert rel_err(direct[n], both[n]) < tol, n
    assert rel_err(both["encoder.vit.blocks.0.mlp.fc1.weight"], fused["encoder.vit.blocks.0.mlp.fc1.weight"]) > 10 * tol  # the probe matters
    # a stale node refuses to run its backward on overwritten activations
    x_enc = model.forward_encoder(images, keep)
    with torch.no_grad():
        model.forward_encoder(images, keep)
    with pytest.raises(RuntimeError, match="overwrote"):
        x_enc.sum().backward()


@pytest.mark.parametrize("prec,tol", [("fp32", 1e-5), ("bf16", 2e-2)])
def test_decoder_embed_decode_predict_compose_to_forward_decoder(dev, prec, tol):
    """src/models/mae.py:57-75 written out with the decoder's own methods."""
    cfg, B = MICRO, 3
    model, params = build(cfg, prec, dev)
    images = O.synthetic_images(B, cfg).to(dev)
    noise = O.make_noise(B, cfg.sequence_length, torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        keep, mask = model.random_token_mask(B, noise)
        x_enc = model.forward_encoder(images, keep)
        want = model.forward_decoder(x_enc, keep, mask)
        Dd, L = cfg.decoder_embed_dim, cfg.sequence_length
        x_decode = model.decoder.embed(x_enc)
        x_masked = model.decoder.mask_token.detach().repeat(B, L, 1)
        x_masked = torch.scatter(x_masked, 1, keep.unsqueeze(-1).expand(-1, -1, Dd), x_decode.type_as(x_masked))
        x_decoded = model.decoder.decode(x_masked)
        x_pred = model.decoder.predict(torch.gather(x_decoded, 1, mask.unsqueeze(-1).expand(-1, -1, Dd)))
    assert x_decode.shape == (B, keep.shape[1], Dd) and x_decoded.shape == (B, L, Dd) and x_pred.shape == want.shape
    assert rel_err(x_pred, want) < tol
    if prec == "fp32":
        ref = O.forward_decoder(params, cfg, x_enc.cpu(), keep.cpu(), mask.cpu())
        assert rel_err(x_pred, ref) < 1e-4
    with pytest.raises(RuntimeError, match="inference call"):
        model.decoder.embed(x_enc)  # grad enabled + trainable decoder: refuses instead of detaching silently
