"""Stochastic depth (drop path) on the host: the scaled reference against the oracle, the draw, the module's key and the CLI flag.
Nothing here needs a GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests import droppath_ref as DR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"
MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)
TINY4 = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=4, num_heads=2))


def _params():
    p = O.init_params(MICRO, 73)
    O.randomize_params(p, seed=5)
    return p


# ---- the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("patch_only", [False, True])
def test_all_ones_table_is_the_oracle(bf16, patch_only):
    p, B = _params(), 3
    images = O.synthetic_images(B, MICRO, seed=4)
    keep = torch.arange(1, MICRO.sequence_length).repeat(B, 1) if patch_only else None
    with torch.no_grad():
        want = O.forward_encoder(p, MICRO, images, idx_keep=keep, bf16=bf16)
        got = DR.forward_encoder(p, MICRO, images, torch.ones(2 * MICRO.depth, B), idx_keep=keep, bf16=bf16)
    assert torch.equal(got, want)


@pytest.mark.parametrize("bf16", [False, True])
def test_dropped_image_is_the_norm_of_its_embedded_tokens(bf16):
    p, B = _params(), 3
    images = O.synthetic_images(B, MICRO, seed=6)
    scale = torch.ones(2 * MICRO.depth, B)
    scale[:, 1] = 0.0
    scale[2, 2] = 2.0
    with torch.no_grad():
        got = DR.forward_encoder(p, MICRO, images, scale, bf16=bf16)
        tok = DR.embedded_tokens(p, MICRO, images, bf16=bf16)
        ones = O.forward_encoder(p, MICRO, images, bf16=bf16)
    want = F.layer_norm(tok[1], (MICRO.embed_dim,), p["encoder.vit.norm.weight"], p["encoder.vit.norm.bias"], O.LN_EPS)
    assert torch.equal(got[1], want)
    assert torch.equal(got[0], ones[0])           # images are independent: image 0 keeps every branch at scale 1
    assert not torch.equal(got[2], ones[2])       # and image 2 has one branch doubled
    with pytest.raises(ValueError):
        DR.forward_encoder(p, MICRO, images, torch.ones(2 * MICRO.depth, B + 1))


def test_scale_reaches_the_gradient():
    """A dropped branch gives its weights no gradient from that image: with every image dropped in block 1's MLP, fc1 / fc2 of block 1 get
    exact zeros and the attention weights of the same block do not."""
    p = {k: v.clone().requires_grad_(True) for k, v in _params().items() if k.startswith("encoder.vit.")}
    B = 2
    scale = torch.ones(2 * MICRO.depth, B)
    scale[3] = 0.0
    DR.forward_encoder(p, MICRO, O.synthetic_images(B, MICRO, seed=1), scale).square().sum().backward()
    assert float(p["encoder.vit.blocks.1.mlp.fc1.weight"].grad.abs().max()) == 0.0
    assert float(p["encoder.vit.blocks.1.mlp.fc2.weight"].grad.abs().max()) == 0.0
    assert float(p["encoder.vit.blocks.1.attn.proj.weight"].grad.abs().max()) > 0.0


# ---- the draw -----------------------------------------------------------------------------------------------------------
def test_draw_is_a_function_of_the_entropy():
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path
    a, b = draw_drop_path(4, 64, 0.3, (73, 0, 5)), draw_drop_path(4, 64, 0.3, (73, 0, 5))
    assert a.dtype == torch.float32 and a.shape == (8, 64) and not a.is_cuda and torch.equal(a, b)
    assert not torch.equal(a, draw_drop_path(4, 64, 0.3, (73, 0, 6)))
    assert not torch.equal(a, draw_drop_path(4, 64, 0.3, (73, 1, 5)))
    g = np.random.default_rng((73, 0, 5))
    assert torch.equal(a, draw_drop_path(4, 64, 0.3, g))   # a Generator is used as it is
    u = np.random.default_rng((73, 0, 5)).random((8, 64))  # kept where u >= p_i
    p = np.repeat(0.3 * np.arange(4) / 3, 2)[:, None]
    assert np.array_equal(a.numpy() != 0, u >= p)


def test_draw_values_and_rates():
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path, drop_path_rates
    assert torch.equal(draw_drop_path(5, 33, 0.0, 1), torch.ones(10, 33))
    assert torch.equal(draw_drop_path(1, 33, 0.9, 1), torch.ones(2, 33))           # depth 1: rate 0
    assert np.allclose(drop_path_rates(12, 0.1), torch.linspace(0, 0.1, 12).double().numpy(), rtol=0, atol=1e-8)
    depth, rate = 4, 0.4
    t = draw_drop_path(depth, 512, rate, 7).numpy()
    assert (t[:2] == 1.0).all()                                                        # block 0 never drops
    for i in range(depth):
        kept = np.float32(1.0 / (1.0 - rate * i / (depth - 1)))
        rows = t[2 * i:2 * i + 2]
        assert set(np.unique(rows).tolist()) <= {0.0, float(kept)}, i
        if i:
            assert (rows == 0).any() and (rows == kept).any()
    assert not np.array_equal(t[2] != 0, t[3] != 0)                                   # the two branches of a block draw independently


def test_kept_counts_within_six_sigma():
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path
    t = draw_drop_path(3, 4096, 0.5, (73, 0, 0)).numpy()
    kept = (t != 0).sum(1)
    assert kept[0] == kept[1] == 4096
    for row in (2, 3):   # p = 0.25: mean 3072, sigma sqrt(4096 * 0.25 * 0.75) = 27.7
        assert abs(int(kept[row]) - 3072) <= 167, kept
    for row in (4, 5):   # p = 0.5: mean 2048, sigma 32
        assert abs(int(kept[row]) - 2048) <= 192, kept
    assert (t[2:4][t[2:4] != 0] == np.float32(1 / 0.75)).all() and (t[4:][t[4:] != 0] == np.float32(2.0)).all()


@pytest.mark.parametrize("rate", [-0.1, 1.0, 1.5, float("nan")])
def test_draw_refuses_a_rate_outside_the_unit_interval(rate):
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path
    with pytest.raises(ValueError):
        draw_drop_path(3, 4, rate, 0)


# ---- module, CLI, symbols -------------------------------------------------------------------------------------------------
def _module(**train):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    vit = encoder_mae(TINY4).encoder.vit
    mc = dict(TINY4, head=dict(embed_dim=32, pool="mean_patches"))
    return ViTClassifierTrainModule(pretrained_encoder=vit, model_cfg=mc, training_cfg=dict({"freeze_encoder": False}, **train))


def test_module_reads_and_validates_drop_path(capsys):
    mod = _module()
    assert mod.drop_path == 0.0 and mod.drop_seed == 73 and mod._drop_step == 0
    assert mod._draw_branch_scale(8) is None and mod._drop_step == 0      # rate 0: nothing is drawn
    mod = _module(drop_path=0.2)
    assert mod.drop_path == 0.2
    t = mod._draw_branch_scale(8)
    assert t.shape == (8, 8) and mod._drop_step == 1
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path
    assert torch.equal(t, draw_drop_path(4, 8, 0.2, (73, 0, 0)))
    mod.current_epoch = 2
    assert torch.equal(mod._draw_branch_scale(8), draw_drop_path(4, 8, 0.2, (73, 2, 1)))
    for bad in (-0.01, 1.0, 3):
        with pytest.raises(ValueError):
            _module(drop_path=bad)
    # a frozen encoder (the linear probe) never drops: the rate is ignored, and said so once
    mod = _module(drop_path=0.2, freeze_encoder=True)
    capsys.readouterr()
    assert mod._draw_branch_scale(8) is None and mod._draw_branch_scale(8) is None and mod._drop_step == 0
    said = capsys.readouterr()
    assert said.err.count("drop_path") == 1 and said.out == ""   # on stderr: the tools print JSON documents on stdout


def test_cli_flag_lands_in_the_train_section():
    import yaml
    from scripts.training import train_mae
    assert train_mae.parse_args([]).drop_path is None
    cfg = {"train": {"learning_rate": 1e-3}}
    train_mae.apply_recipe_flags(cfg, train_mae.parse_args(["--drop_path", "0.1"]))
    assert cfg["train"] == {"learning_rate": 1e-3, "drop_path": 0.1}
    cfg2 = {"train": {"drop_path": 0.2, "mixup_alpha": 0.8}}
    train_mae.apply_recipe_flags(cfg2, train_mae.parse_args([]))
    assert cfg2 == {"train": {"drop_path": 0.2, "mixup_alpha": 0.8}}   # no flag, no change
    ft = yaml.safe_load((ROOT / "configs" / "vits8_dec192_finetune.yaml").read_text())
    assert "drop_path" not in ft["train"]                                # the committed recipe's runs do not change
    assert '"--drop_path"' in (ROOT / "tools" / "classifier_bench.py").read_text()


def test_new_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for n in ("mae_engine_classifier_loss_and_grads_sd", "mae_add_layernorm_fwd_scaled", "mae_layernorm_bwd_scaled"):
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.ABI_VERSION == 4 and _lib.lib.mae_abi_version() == 4  # additive
    S = _lib.SIGNATURES
    assert len(S["mae_engine_classifier_loss_and_grads_sd"][1]) == len(S["mae_engine_classifier_loss_and_grads_soft"][1]) + 1
    assert len(S["mae_add_layernorm_fwd_scaled"][1]) == len(S["mae_add_layernorm_fwd"][1]) + 2
    assert len(S["mae_layernorm_bwd_scaled"][1]) == len(S["mae_layernorm_bwd"][1]) + 2


def test_scaled_calls_refuse_bad_arguments_before_any_launch():
    """rows_per_image <= 0 is an error of the call itself: it returns before anything touches a device (no GPU here)."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    one = 1 << 12   # never dereferenced: the argument checks come first
    for rpi in (0, -3):
        assert lib.mae_add_layernorm_fwd_scaled(one, one, one, None, one, one, 1e-6, 4, 8, 0, one, one, one, one, rpi, None) != 0
        assert b"rows_per_image" in lib.mae_last_error()
        assert lib.mae_layernorm_bwd_scaled(one, 0, one, None, one, one, one, 4, 8, 0, one, one, one, one, one, one, rpi, None) != 0
        assert b"rows_per_image" in lib.mae_last_error()
    assert lib.mae_layernorm_bwd_scaled(one, 0, one, None, one, one, one, 4, 8, 0, one, None, one, one, one, one, 4, None) != 0
    assert b"dx_copy" in lib.mae_last_error()
