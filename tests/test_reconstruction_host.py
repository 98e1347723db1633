"""Reconstruction evaluation without a GPU: the CPU reference against hand-written answers, the statistics formulas, checkpoint
layouts and strict loading on CPU state dicts, the CLI's arguments, the figure writer and the C ABI names."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import recon_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"

NEW_SYMBOLS = ("mae_reconstruct_scratch_bytes", "mae_reconstruct_compose", "mae_engine_reconstruct")
TINY = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=1, num_heads=2),
            decoder=dict(decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2))


def test_new_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.ABI_VERSION == 4 and "#define MAE_ABI_VERSION 4" in HEADER.read_text()


def test_scratch_metadata():
    from ssrl_vit_mae_jepa_amd import _lib
    f = _lib.lib.mae_reconstruct_scratch_bytes
    assert f(2000, 3, 96, 8) >= 2000 * 144 * 4 and f(1, 1, 30, 6) > 0
    for bad in ((0, 3, 96, 8), (4, 3, 96, 7), (4, 3, 96, 0), (4, 0, 96, 8), (1 << 30, 3, 96, 8)):
        assert f(*bad) == -1, bad


def test_recon_ref_known_answer_2x2_patches():
    """One 4x4 one-channel image, p = 2: tokens 2 and 4 (patches 1 and 3, the right column) are replaced."""
    img = torch.arange(16, dtype=torch.float32).view(1, 1, 4, 4)
    pred = torch.tensor([[[10., 11., 12., 13.], [20., 21., 22., 23.]]])
    recon, masked = R.compose_ref(img, pred, torch.tensor([[2, 4]]), 2, fill=0.5)
    assert torch.equal(recon[0, 0], torch.tensor([[0., 1., 10., 11.], [4., 5., 12., 13.], [8., 9., 20., 21.], [12., 13., 22., 23.]]))
    assert torch.equal(masked[0, 0], torch.tensor([[0., 1., .5, .5], [4., 5., .5, .5], [8., 9., .5, .5], [12., 13., .5, .5]]))
    sq, ab = R.sums_ref(img, recon)
    # differences: patch 1 -> 10-2, 11-3, 12-6, 13-7 = 8, 8, 6, 6; patch 3 -> 20-10, 21-11, 22-14, 23-15 = 10, 10, 8, 8
    assert sq.tolist() == [2 * 64 + 2 * 36 + 2 * 100 + 2 * 64] and ab.tolist() == [16 + 12 + 20 + 16]
    # the class token (0) and an id past the grid (5) are dropped together with their pred rows
    recon2, masked2 = R.compose_ref(img, torch.cat([pred, pred + 100], 1), torch.tensor([[2, 0, 4, 5]]), 2)
    want = recon.clone()
    want[0, 0, 2:, 2:] = torch.tensor([[110., 111.], [112., 113.]])
    assert torch.equal(recon2, want) and torch.equal(masked2, masked)


def test_recon_ref_channel_order_and_display():
    """per-patch order (py, px, c): one 2x2 two-channel patch."""
    img = torch.zeros(1, 2, 2, 2)
    pred = torch.arange(8, dtype=torch.float32).view(1, 1, 8)
    recon, _ = R.compose_ref(img, pred, torch.tensor([[1]]), 2)
    for c in range(2):
        for y in range(2):
            for x in range(2):
                assert recon[0, c, y, x] == (y * 2 + x) * 2 + c
    u8 = torch.tensor([0, 1, 127, 128, 254, 255], dtype=torch.uint8)
    assert torch.equal(R.display_u8(R.normalize_u8(u8)), u8)  # display inverts the normalisation on every pixel value
    assert torch.equal(R.display_u8(R.normalize_u8(torch.arange(256, dtype=torch.uint8))), torch.arange(256, dtype=torch.uint8))
    assert R.display_u8(torch.tensor([-3.0, 3.0, 0.0])).tolist() == [0, 255, 128]  # clamp; 127.5 rounds half to even


def test_reconstruction_stats_match_torch_losses():
    from ssrl_vit_mae_jepa_amd.reconstruction import reconstruction_stats
    g = torch.Generator().manual_seed(3)
    B, C, S, p, m = 4, 3, 16, 4, 5
    img = torch.rand(B, C, S, S, generator=g) * 2 - 1
    pred = torch.randn(B, m, p * p * C, generator=g)
    idx = torch.stack([torch.randperm(16, generator=g)[:m] + 1 for _ in range(B)])
    recon, _ = R.compose_ref(img, pred, idx, p)
    sq, ab = R.sums_ref(img, recon)
    st = reconstruction_stats(sq, ab, C * S * S, m * p * p * C)
    mse = torch.nn.functional.mse_loss(recon.double(), img.double()).item()
    l1 = torch.nn.functional.l1_loss(recon.double(), img.double()).item()
    assert st["images"] == B
    assert math.isclose(st["mse"], mse, rel_tol=1e-6) and math.isclose(st["l1"], l1, rel_tol=1e-6)
    assert math.isclose(st["psnr"], -10 * math.log10(mse), rel_tol=1e-6)
    target = torch.gather(R.O.patchify(img, p), 1, (idx - 1).unsqueeze(-1).expand(-1, -1, p * p * C))
    assert math.isclose(st["masked_mse"], torch.nn.functional.mse_loss(pred.double(), target.double()).item(), rel_tol=1e-6)
    with pytest.raises(ValueError):
        reconstruction_stats(sq, ab[:2], C * S * S, 10)
    with pytest.raises(ValueError):
        reconstruction_stats(sq, ab, 10, 11)


def _mae_state(seed):
    from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
    m = MaskedAutoencoder(TINY["general"], TINY["encoder"], TINY["decoder"])
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in m.state_dict().items()}


def test_load_mae_checkpoint_layouts(tmp_path):
    from ssrl_vit_mae_jepa_amd.reconstruction import load_mae_checkpoint
    sd = _mae_state(1)
    lightning = {"state_dict": {f"model.{k}": v for k, v in sd.items()}, "epoch": 3, "global_step": 7}
    torch.save(lightning, tmp_path / "last.ckpt")   # what pretrain_mae's save_checkpoint writes
    torch.save(sd, tmp_path / "vit-mae.pt")         # what pretrain_mae writes at the end
    cases = ((lightning, "state_dict"), ({"model_state_dict": sd}, "model_state_dict"), (sd, "raw"),
             ({f"model.{k}": v for k, v in sd.items()}, "raw"), (tmp_path / "last.ckpt", "state_dict"), (str(tmp_path / "vit-mae.pt"), "raw"))
    for src, layout in cases:
        model, found = load_mae_checkpoint(src, TINY)
        assert found == layout
        got = model.state_dict()
        assert set(got) == set(sd)
        for k, v in sd.items():
            assert torch.equal(got[k], v), k
    assert load_mae_checkpoint(sd, TINY, precision="bf16")[0].engine.precision == "bf16"
    with pytest.raises(FileNotFoundError):
        load_mae_checkpoint(tmp_path / "missing.ckpt", TINY)


def test_load_mae_checkpoint_is_strict():
    from ssrl_vit_mae_jepa_amd.reconstruction import load_mae_checkpoint
    sd = _mae_state(2)
    lacking = {k: v for k, v in sd.items() if k != "decoder.decoder_pred.weight"}
    with pytest.raises(ValueError, match="missing.*decoder.decoder_pred.weight"):
        load_mae_checkpoint({"state_dict": {f"model.{k}": v for k, v in lacking.items()}}, TINY)
    with pytest.raises(ValueError, match="unexpected.*head.weight"):
        load_mae_checkpoint({**sd, "head.weight": torch.zeros(10, 32)}, TINY)
    with pytest.raises(ValueError):
        load_mae_checkpoint({"state_dict": {}}, TINY)


def test_cli_arguments():
    from scripts.evaluation import visualize_reconstruction as V
    a = V.parse_args([])
    # the reference's three flags and their defaults (scripts/evaluation/visualize_reconstruction.py:29-50)
    assert (a.config, a.model_path, a.output_path_suffix) == ("configs/mae.yaml", "outputs/pretrain/mae_100/checkpoints/best.ckpt",
                                                              "reconstruction_validation.png")
    assert (a.synthetic_images, a.num_samples, a.mask_seed, a.batch_size, a.eval_split) == (None, 8, 42, None, "none")
    assert Path(a.output_dir) == Path("assets") / "visualizations"
    a = V.parse_args(["--model_path", "random", "--synthetic_images", "16", "--num_samples", "4", "--eval_split", "val", "--mask_seed", "7",
                      "--batch_size", "32", "--output_dir", "x", "--config", "configs/vits8_dec192.yaml", "--output_path_suffix", "r.png"])
    assert (a.model_path, a.synthetic_images, a.num_samples, a.eval_split, a.mask_seed, a.batch_size, a.output_dir, a.output_path_suffix) == \
        ("random", 16, 4, "val", 7, 32, "x", "r.png")
    with pytest.raises(SystemExit):
        V.parse_args(["--eval_split", "test"])


def test_figure_writer(tmp_path):
    from ssrl_vit_mae_jepa_amd.reconstruction import save_reconstruction_figure, to_display_u8
    g = torch.Generator().manual_seed(5)
    a, b, c = (torch.randint(0, 256, (2, 3, 16, 16), generator=g, dtype=torch.uint8) for _ in range(3))
    out = save_reconstruction_figure(a, b.numpy(), c, tmp_path / "sub" / "fig.png", mask_ratio=0.75)
    assert out.exists() and out.stat().st_size > 1000 and out.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    save_reconstruction_figure(a[:1, :1], b[:1, :1], c[:1, :1], tmp_path / "one.png")  # one image, one channel
    assert (tmp_path / "one.png").stat().st_size > 0
    with pytest.raises(ValueError):
        save_reconstruction_figure(a, b[:1], c, tmp_path / "bad.png")
    with pytest.raises(ValueError):
        save_reconstruction_figure(a.float(), b, c, tmp_path / "bad.png")
    x = torch.rand(2, 3, 4, 4, generator=g) * 3 - 1.5
    assert torch.equal(to_display_u8(x), R.display_u8(x)) and to_display_u8(a) is a
    assert np.asarray(to_display_u8(x)).dtype == np.uint8
