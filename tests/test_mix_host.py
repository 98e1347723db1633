"""Host-side checks (no GPU) of the fine-tuning recipe: the soft-target reference against torch's cross-entropy, the mixup /
CutMix draw, the layer numbering and learning-rate scales of layer-wise decay, the new symbols, keys and flags."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mix_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"
TINY4 = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=4, num_heads=2))


# ---- the soft-target reference --------------------------------------------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("lam", [0.0, 0.3, 1.0])
def test_soft_reference_is_the_torch_combination(lam, eps):
    g = torch.Generator().manual_seed(5)
    B, C = 7, 10
    ya, yb = torch.randint(0, C, (B,), generator=g), torch.randint(0, C, (B,), generator=g)
    yb[2] = ya[2]  # a pair of equal labels
    lam_v = torch.full((B,), lam, dtype=torch.float32)
    lam64 = lam_v.double()  # 0.3 as the fp32 value both sides use
    for same in (False, True):
        b = ya if same else yb
        logits = torch.randn(B, C, generator=g, dtype=torch.float64, requires_grad=True)
        loss = R.soft_loss(logits, ya, b, lam_v, eps)
        grad, = torch.autograd.grad(loss, logits)
        ref_logits = logits.detach().clone().requires_grad_(True)
        rows = lam64 * F.cross_entropy(ref_logits, ya, label_smoothing=eps, reduction="none") + \
            (1 - lam64) * F.cross_entropy(ref_logits, b, label_smoothing=eps, reduction="none")
        ref = rows.mean()
        ref_grad, = torch.autograd.grad(ref, ref_logits)
        assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-13 * abs(float(ref.detach()))
        assert float((grad - ref_grad).abs().max()) <= 1e-15
        # the closed form the kernel uses: (softmax - t) / B
        t = R.soft_targets(ya, b, lam_v, eps, C)
        assert float(t.sum(1).sub(1).abs().max()) <= 1e-15
        assert float(((torch.softmax(logits.detach(), 1) - t) / B - ref_grad).abs().max()) <= 1e-15


def test_soft_head_reference_reduces_to_the_hard_one():
    g = torch.Generator().manual_seed(3)
    B, rows, D, C = 5, 6, 16, 4
    feats, head = torch.randn(B, rows, D, generator=g), torch.randn(C * D + C, generator=g) * 0.2
    y = torch.randint(0, C, (B,), generator=g)
    logits, loss, correct, hg, df = R.soft_head_reference(feats, "mean", 0, head, C, y, y, torch.ones(B), 0.0, False, grad_scale=0.5)
    assert abs(float(loss) - float(F.cross_entropy(logits, y))) <= 1e-14
    dl = (torch.softmax(logits, 1) - F.one_hot(y, C).double()) * 0.5 / B
    assert float((hg[C * D:] - dl.sum(0)).abs().max()) <= 1e-8 and df.shape == (B, rows, D)  # d_logits is held in fp32
    assert correct == int((logits.argmax(1) == y).sum())


# ---- the draw -------------------------------------------------------------------------------------------------------
def test_draw_is_deterministic_in_its_seed_and_well_formed():
    from ssrl_vit_mae_jepa_amd.data import draw_mix_params
    B, S = 7, 96
    seen_cutmix = seen_mixup = False
    for step in range(40):
        a = draw_mix_params(B, S, (73, 2, step), 0.8, 1.0, 1.0, 0.5)
        b = draw_mix_params(B, S, (73, 2, step), 0.8, 1.0, 1.0, 0.5)
        assert a.cutmix == b.cutmix and all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
        assert a.partner.dtype == torch.int32 and a.lam.dtype == torch.float32 and a.box.dtype == torch.int32
        assert a.partner.tolist() == list(range(B - 1, -1, -1))  # the flipped batch; the middle image is its own partner
        assert a.box.shape == (B, 4) and a.lam.shape == (B,)
        y0, y1, x0, x1 = a.box[0].tolist()
        assert 0 <= y0 <= y1 <= S and 0 <= x0 <= x1 <= S and bool((a.box == a.box[0]).all()) and bool((a.lam == a.lam[0]).all())
        if a.cutmix:
            seen_cutmix = True
            area = (y1 - y0) * (x1 - x0)
            assert a.lam[0].item() == float(np.float32(1.0 - area / float(S * S)))  # corrected to the box that was cut
        else:
            seen_mixup = True
            assert (y0, y1, x0, x1) == (0, 0, 0, 0) and 0.0 <= a.lam[0].item() <= 1.0
    assert seen_cutmix and seen_mixup
    c = draw_mix_params(B, S, (73, 3, 0), 0.8, 1.0, 1.0, 0.5)
    d = draw_mix_params(B, S, (73, 2, 0), 0.8, 1.0, 1.0, 0.5)
    assert not (torch.equal(c.lam, d.lam) and torch.equal(c.box, d.box))  # another epoch, another draw
    # a passed-in generator advances
    rng = np.random.default_rng(1)
    e, f = draw_mix_params(B, S, rng, 0.8, 0.0), draw_mix_params(B, S, rng, 0.8, 0.0)
    assert not e.cutmix and not f.cutmix and not torch.equal(e.lam, f.lam)


def test_draw_box_follows_the_cut_ratio():
    """cut = int(S * sqrt(1 - lam0)) and edges clip(c -+ cut // 2, 0, S): replay the generator's stream."""
    from ssrl_vit_mae_jepa_amd.data import draw_mix_params
    S = 96
    for seed in range(20):
        p = draw_mix_params(4, S, seed, 0.0, 1.0, 1.0, 0.5)  # cutmix alone
        assert p.cutmix
        rng = np.random.default_rng(seed)
        assert rng.random() < 1.0
        lam0 = float(rng.beta(1.0, 1.0))
        cut = int(S * math.sqrt(1.0 - lam0))
        cy, cx = int(rng.integers(0, S)), int(rng.integers(0, S))
        want = [int(np.clip(cy - cut // 2, 0, S)), int(np.clip(cy + cut // 2, 0, S)), int(np.clip(cx - cut // 2, 0, S)), int(np.clip(cx + cut // 2, 0, S))]
        assert p.box[0].tolist() == want


def test_draw_prob_zero_is_the_identity_and_switch_share():
    from ssrl_vit_mae_jepa_amd.data import draw_mix_params
    for seed in range(10):
        p = draw_mix_params(6, 32, seed, 0.8, 1.0, 0.0, 0.5)
        assert p.identity and not p.cutmix and bool((p.lam == 1).all()) and bool((p.box == 0).all())
    assert draw_mix_params(6, 32, 0, 0.0, 0.0, 1.0, 0.5).identity  # nothing configured
    # 2000 seeded draws: the CutMix share is a binomial with sigma = sqrt(.25 / 2000) = 0.0112; 0.05 is 4.5 sigma
    rng = np.random.default_rng(73)
    share = sum(draw_mix_params(2, 32, rng, 0.8, 1.0, 1.0, 0.5).cutmix for _ in range(2000)) / 2000.0
    assert abs(share - 0.5) <= 0.05, share
    assert all(draw_mix_params(2, 32, s, 0.8, 0.0).cutmix is False for s in range(5))
    assert all(draw_mix_params(2, 32, s, 0.0, 1.0).cutmix is True for s in range(5))


# ---- layer-wise learning-rate decay ---------------------------------------------------------------------------------
def _module(layer_decay=1.0, with_cls=True, **train):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    vit = encoder_mae(TINY4).encoder.vit
    vit.with_cls = with_cls
    mc = dict(TINY4, head=dict(embed_dim=32, pool="mean_patches"))
    return ViTClassifierTrainModule(pretrained_encoder=vit, model_cfg=mc, training_cfg=dict(freeze_encoder=False, layer_decay=layer_decay, **train))


def test_layer_numbering_and_scales_depth_4():
    mod = _module(0.5)
    want = {"cls_token": 0, "pos_embed": 0, "patch_embed.proj.weight": 0, "patch_embed.proj.bias": 0, "blocks.0.norm1.weight": 1,
            "blocks.0.mlp.fc2.bias": 1, "blocks.3.attn.qkv.weight": 4, "norm.weight": 5, "norm.bias": 5, "head": 5}
    for name, layer in want.items():
        assert mod.layer_of(name) == layer, name
        assert mod.layer_scale(layer) == 0.5 ** (5 - layer)
    assert {mod.layer_of(n) for n, _ in mod.model.encoder.named_parameters()} == set(range(6))
    assert mod.layer_scale(5) == 1.0 and mod.layer_scale(0) == 0.5 ** 5


@pytest.mark.parametrize("with_cls", [True, False])
def test_decay_groups_cut_at_the_block_boundaries(with_cls):
    mod = _module(0.5, with_cls)
    m = mod.model.mae
    depth = 4
    for tb, te in ((-1, 0), (0, 0), (1, 0), (3, 0), (4, 0), (4, 1)):
        pieces, row0 = mod._update_ranges(tb, te)
        groups, grow0 = mod._decay_groups(tb, te)
        assert grow0 == row0
        # the groups tile exactly the pieces, in order
        assert sorted((lo, lo + n) for lo, n, _s in groups) == [(lo, lo + n) for lo, n, _s in groups]
        covered = [(lo, lo + n) for lo, n, _s in groups]
        merged = []
        for a, b in covered:
            if merged and merged[-1][1] == a:
                merged[-1] = (merged[-1][0], b)
            else:
                merged.append((a, b))
        assert merged == [(lo, lo + n) for lo, n in pieces]
        assert all(lo % 4 == 0 and n % 4 == 0 and n > 0 for lo, n, _s in groups)  # what mae_engine_adamw_range asks for
        # every trainable arena tensor lies inside one group, whose scale is its layer's
        for name, off, numel, _shape, _f in m.engine.table:
            if not name.startswith("encoder.vit.") or name.endswith("pos_embed"):
                continue
            inside = [s for lo, n, s in groups if lo <= off and off + numel <= lo + n]
            touched = any(lo < off + numel and off < lo + n for lo, n, _s in groups)
            if touched:
                assert inside == [mod.layer_scale(mod.layer_of(name[len("encoder.vit."):]))], name
        if tb >= 0:
            assert len({s for _lo, _n, s in groups}) == tb + 1 + te
        else:
            assert groups == []


@pytest.mark.parametrize("with_cls", [True, False])
def test_layer_decay_one_is_todays_ranges(with_cls):
    mod = _module(1.0, with_cls)
    for tb, te in ((-1, 0), (0, 0), (2, 0), (4, 0), (4, 1)):
        pieces, row0 = mod._update_ranges(tb, te)
        assert mod._decay_groups(tb, te) == ([(lo, n, 1.0) for lo, n in pieces], row0)
    assert mod.layer_scale(0) == 1.0  # pos_embed's learning rate is lr * 1.0: the same float


# ---- keys, flags, symbols ---------------------------------------------------------------------------------------------
def test_module_reads_the_recipe_keys_and_defaults_are_off():
    mod = _module()
    assert (mod.label_smoothing, mod.mixup_alpha, mod.cutmix_alpha, mod.mix_prob, mod.mix_switch_prob, mod.layer_decay) == (0.0, 0.0, 0.0, 1.0, 0.5, 1.0)
    mod = _module(0.75, label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0, mix_prob=0.9, mix_switch_prob=0.4)
    assert (mod.label_smoothing, mod.mixup_alpha, mod.cutmix_alpha, mod.mix_prob, mod.mix_switch_prob, mod.layer_decay) == (0.1, 0.8, 1.0, 0.9, 0.4, 0.75)
    with pytest.raises(ValueError):
        _module(label_smoothing=1.0)
    with pytest.raises(ValueError):
        _module(1.5)


def test_cli_flags_override_the_yaml_and_finetune_config():
    import yaml
    from scripts.training import train_mae
    a = train_mae.parse_args([])
    assert (a.label_smoothing, a.mixup, a.cutmix, a.layer_decay) == (None, None, None, None)
    a = train_mae.parse_args(["--label_smoothing", "0.1", "--mixup", "0.8", "--cutmix", "1.0", "--layer_decay", "0.75"])
    cfg = {"train": {"label_smoothing": 0.0, "learning_rate": 1e-3}}
    train_mae.apply_recipe_flags(cfg, a)
    assert cfg["train"] == {"label_smoothing": 0.1, "mixup_alpha": 0.8, "cutmix_alpha": 1.0, "layer_decay": 0.75, "learning_rate": 1e-3}
    cfg2 = {"train": {"mixup_alpha": 0.2}}
    train_mae.apply_recipe_flags(cfg2, train_mae.parse_args([]))
    assert cfg2 == {"train": {"mixup_alpha": 0.2}}  # no flag, no change
    ft = yaml.safe_load((ROOT / "configs" / "vits8_dec192_finetune.yaml").read_text())
    t = ft["train"]
    assert (t["label_smoothing"], t["mixup_alpha"], t["cutmix_alpha"], t["layer_decay"]) == (0.1, 0.8, 1.0, 0.75)
    assert t["freeze_encoder"] is False and ft["model"]["head"]["pool"] == "mean_patches"
    base = yaml.safe_load((ROOT / "configs" / "vits8_dec192.yaml").read_text())
    assert ft["model"]["encoder"] == base["model"]["encoder"] and ft["model"]["general"] == base["model"]["general"]


def test_new_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for n in ("mae_classifier_head_soft", "mae_engine_classifier_loss_and_grads_soft", "mae_mix_batch"):
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.ABI_VERSION == 4 and _lib.lib.mae_abi_version() == 4  # additive
    # labels_b, lam, label_smoothing in front of the stream
    for soft, ex in (("mae_classifier_head_soft", "mae_classifier_head_ex"),
                     ("mae_engine_classifier_loss_and_grads_soft", "mae_engine_classifier_loss_and_grads_ex")):
        assert len(_lib.SIGNATURES[soft][1]) == len(_lib.SIGNATURES[ex][1]) + 3


def test_mix_reference_properties():
    """The fp64 mix reference on a hand-made case: inside pixels are the partner's, lam == 1 is a copy, the bound is zero there."""
    g = np.random.default_rng(0)
    img = g.integers(0, 256, (3, 1, 4, 4), dtype=np.uint8)
    ref, bound, exact = R.mix_reference(img, [2, 7, 0], [0.25, 0.5, 1.0], [[1, 3, 0, 2], [0, 0, 0, 0], [0, 9, -3, 1]])
    n = R.normalize_u8_f32(img).astype(np.float64)
    assert np.array_equal(ref[0, 0, 1:3, 0:2], n[2, 0, 1:3, 0:2]) and exact[0, 0, 1:3, 0:2].all() and not exact[0, 0, 0].any()
    assert np.allclose(ref[0, 0, 0], 0.25 * n[0, 0, 0] + 0.75 * n[2, 0, 0], rtol=0, atol=1e-15)
    assert np.array_equal(ref[1], n[1])  # partner 7 is out of range: the image mixes with itself (to fp64 rounding: lam a + (1 - lam) a)
    assert np.array_equal(ref[2, 0, :, 1:], n[2, 0, :, 1:]) and np.array_equal(ref[2, 0, :, 0], n[0, 0, :, 0]) and exact[2].all()
    assert (bound[exact] == 0).all() and (bound[~exact] > 0).all()
    assert np.array_equal(R.cutmix_u8_reference(img, [2, 7, 0], [[1, 3, 0, 2], [0, 0, 0, 0], [0, 9, -3, 1]])[0, 0, 1:3, 0:2], img[2, 0, 1:3, 0:2])
