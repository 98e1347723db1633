"""Normalised-pixel targets (norm_pix_loss) without a GPU: the flag on the model and in the engine's config, the rejected
combination with latent targets, the flag's way through checkpoints and the pretrain CLI, the C ABI names, and the float64
reference of the GPU tests against a hand-written loop."""
import ctypes as C
import math
import re
from pathlib import Path

import pytest
import torch

from tests import normpix_ref as NR

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"
NEW_SYMBOLS = ("mae_patchify_gather_norm", "mae_mse_loss_norm_pix", "mae_norm_pix_restore")
ENC = dict(embed_dim=32, depth=1, num_heads=2)
DEC = dict(decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2)


def general(**kw):
    return dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32", **kw)


def test_symbols_config_layout_and_eps():
    from ssrl_vit_mae_jepa_amd import _lib
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.ABI_VERSION == 4 and "#define MAE_ABI_VERSION 4" in raw
    assert re.search(r"#define\s+MAE_NORM_PIX_EPS\s+1e-6\b", text) and _lib.NORM_PIX_EPS == NR.EPS == 1e-6
    assert re.search(r"int32_t\s+norm_pix_loss\s*;\s*int32_t\s+reserved\[3\]\s*;", text)
    # same size, the flag sits where reserved[0] sat
    assert C.sizeof(_lib.MaeConfig) == 16 * 4 and _lib.MaeConfig.norm_pix_loss.offset == 12 * 4 and _lib.MaeConfig.reserved.offset == 13 * 4


def test_flag_on_the_model_changes_no_engine_metadata():
    from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
    on = MaskedAutoencoder(general(norm_pix_loss=True), ENC, DEC)
    off = MaskedAutoencoder(general(), ENC, DEC)
    assert on.norm_pix_loss is True and off.norm_pix_loss is False
    assert MaskedAutoencoder(general(norm_pix_loss=False), ENC, DEC).norm_pix_loss is False
    for attr in ("arena_elems", "trainable_elems", "wcache_bytes", "table"):
        assert getattr(on.engine, attr) == getattr(off.engine, attr), attr
    for batch, keep in ((1, 1), (4, 4), (7, 16)):
        assert on.engine.workspace_bytes(batch, keep) == off.engine.workspace_bytes(batch, keep) > 0
    assert list(on.state_dict()) == list(off.state_dict())


def test_engine_rejects_the_flag_with_latent_targets():
    from ssrl_vit_mae_jepa_amd import MaskedAutoencoder, _lib
    with pytest.raises(ValueError, match="norm_pix_loss"):
        MaskedAutoencoder(general(norm_pix_loss=True, pred_dim=32), ENC, DEC)
    MaskedAutoencoder(general(pred_dim=32), ENC, DEC)  # the I-JEPA engine itself is fine
    cfg = _lib.MaeConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=32, depth=1, num_heads=2, decoder_embed_dim=32, decoder_depth=1,
                         decoder_num_heads=2, mlp_ratio=4, act_dtype=_lib.MAE_F32, pred_dim=32, norm_pix_loss=1)
    h = C.c_void_p()
    assert _lib.lib.mae_engine_create(C.byref(cfg), C.byref(h)) != 0 and not h.value
    assert b"norm_pix_loss" in _lib.lib.mae_last_error()


def test_flag_round_trips_through_checkpoints(capsys):
    from ssrl_vit_mae_jepa_amd import MAEPretrainModule
    from ssrl_vit_mae_jepa_amd.reconstruction import checkpoint_norm_pix_loss, load_mae_checkpoint
    tcfg = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=8, warmup_epochs=2, batch_size=32,
                base_learning_rate=1.5e-4, weight_decay=0.05)
    absent = dict(general=general(), encoder=ENC, decoder=DEC)
    with_flag = dict(absent, general=general(norm_pix_loss=True))
    without = dict(absent, general=general(norm_pix_loss=False))
    ck_on = MAEPretrainModule(with_flag, tcfg).checkpoint_dict(0)
    ck_off = MAEPretrainModule(without, tcfg).checkpoint_dict(0)
    ck_silent = MAEPretrainModule(absent, tcfg).checkpoint_dict(0)
    assert checkpoint_norm_pix_loss(ck_on) is True and checkpoint_norm_pix_loss(ck_off) is False
    assert checkpoint_norm_pix_loss(ck_silent) is None and checkpoint_norm_pix_loss(ck_on["state_dict"]) is None

    # the checkpoint's value wins over an absent key, and says so in one line
    capsys.readouterr()
    model, layout = load_mae_checkpoint(ck_on, absent)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if "norm_pix_loss" in ln]
    assert model.norm_pix_loss is True and layout == "state_dict" and len(lines) == 1 and "checkpoint" in lines[0]
    assert "norm_pix_loss" not in absent["general"]  # the caller's config is not modified
    assert load_mae_checkpoint(ck_off, absent)[0].norm_pix_loss is False
    assert load_mae_checkpoint(ck_on, with_flag)[0].norm_pix_loss is True
    capsys.readouterr()
    assert load_mae_checkpoint(ck_silent, absent)[0].norm_pix_loss is False and "norm_pix_loss" not in capsys.readouterr().out
    # a conflict raises, either way round
    with pytest.raises(ValueError, match="norm_pix_loss"):
        load_mae_checkpoint(ck_on, without)
    with pytest.raises(ValueError, match="norm_pix_loss"):
        load_mae_checkpoint(ck_off, with_flag)
    # a bare state dict carries no flag: the config decides
    bare = {k[len("model."):]: v for k, v in ck_on["state_dict"].items()}
    assert load_mae_checkpoint(bare, absent)[0].norm_pix_loss is False
    m, layout = load_mae_checkpoint(bare, with_flag)
    assert m.norm_pix_loss is True and layout == "raw"


def test_pretrain_cli_flag_overrides_the_config():
    import yaml
    from scripts.evaluation import visualize_reconstruction as V
    from scripts.training import pretrain_mae as cli
    cfg = yaml.safe_load(open(ROOT / "configs" / "vits8_dec192.yaml"))
    assert "norm_pix_loss" not in cfg["model"]["general"]
    assert cli.apply_overrides(cfg, cli.parse_args([])) == cfg and cli.parse_args([]).norm_pix_loss is False
    over = cli.apply_overrides(cfg, cli.parse_args(["--norm_pix_loss"]))
    assert over["model"]["general"]["norm_pix_loss"] is True and "norm_pix_loss" not in cfg["model"]["general"]
    assert {k: v for k, v in over["model"]["general"].items() if k != "norm_pix_loss"} == cfg["model"]["general"]
    false_cfg = dict(cfg, model=dict(cfg["model"], general=dict(cfg["model"]["general"], norm_pix_loss=False)))
    assert cli.apply_overrides(false_cfg, cli.parse_args(["--norm_pix_loss"]))["model"]["general"]["norm_pix_loss"] is True
    # the shipped config is vits8_dec192 with the key set, nothing else
    shipped = yaml.safe_load(open(ROOT / "configs" / "vits8_dec192_normpix.yaml"))
    assert shipped == over
    assert V.parse_args(["--norm_pix_loss"]).norm_pix_loss is True and V.parse_args([]).norm_pix_loss is False


def test_reference_against_a_hand_written_loop():
    """One 4x4 two-channel image, p = 2: token 3 is patch 2 (rows 2-3, columns 0-1); per-patch order (py, px, c)."""
    img = torch.arange(32, dtype=torch.float32).view(1, 2, 4, 4) / 16 - 1
    t, mean, rstd = NR.target_ref(img, torch.tensor([[3]]), 2)
    x = [float(img[0, c, 2 + py, px]) for py in range(2) for px in range(2) for c in range(2)]
    mu = sum(x) / 8
    var = sum((v - mu) ** 2 for v in x) / 7
    want = [(v - mu) / math.sqrt(var + 1e-6) for v in x]
    assert t.dtype == torch.float64 and t.shape == (1, 1, 8)
    assert max(abs(a - b) for a, b in zip(t[0, 0].tolist(), want)) < 1e-14
    assert abs(float(mean) - mu) < 1e-15 and abs(float(rstd) - 1 / math.sqrt(var + 1e-6)) < 1e-12
    loss, d = NR.loss_ref(torch.zeros(1, 1, 8), img, torch.tensor([[3]]), 2, grad_scale=0.5)
    assert abs(loss - sum(w * w for w in want) / 8) < 1e-14
    assert max(abs(a + 0.5 * 2 * w / 8) for a, w in zip(d[0, 0].tolist(), want)) < 1e-15
    # uint8 pixels are normalised first
    u8 = torch.randint(0, 256, (1, 2, 4, 4), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    assert torch.equal(NR.target_ref(u8, torch.tensor([[1, 4]]), 2)[0], NR.target_ref(NR.normalize_u8(u8), torch.tensor([[1, 4]]), 2)[0])


def test_reference_constant_patch_is_exactly_zero():
    for img in (torch.full((1, 3, 4, 4), 37, dtype=torch.uint8), torch.full((1, 1, 4, 4), -0.3)):
        t, _mean, rstd = NR.target_ref(img, torch.tensor([[1, 2, 3, 4]]), 2)
        assert torch.equal(t, torch.zeros_like(t)) and torch.equal(rstd, torch.full_like(rstd, 1 / math.sqrt(1e-6)))
