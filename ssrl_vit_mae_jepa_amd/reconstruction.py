"""What a pretrained MAE reconstructs: the reference's ``scripts/evaluation/visualize_reconstruction.py`` (``MAEReconstructor``)
over the engine, plus the same statistics accumulated over a whole split.

The model forward, the masked / reconstructed images and the per-image error sums come from ONE native call
(``MaskedAutoencoder.reconstruct`` -> ``mae_engine_reconstruct``); the host only turns the per-image sums into MSE / L1 / PSNR
(float64), loads checkpoints and draws the figure.
"""
from __future__ import annotations

import math
from pathlib import Path
from typing import Any, Dict, Iterable, Optional, Tuple, Union

import torch

from .data import normalize_u8
from .mae import MaskedAutoencoder

MASK_SEED = 42  # torch.manual_seed(42) in front of the reference's mask draw (visualize_reconstruction.py:150)


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def mae_state_dict(ckpt: Any) -> Tuple[Dict[str, torch.Tensor], str]:
    """(state dict with the ``model.`` prefix removed, layout name) of a loaded checkpoint -- the three formats the reference
    sniffs (visualize_reconstruction.py:102-117): ``state_dict`` (a Lightning checkpoint: this repository's ``last.ckpt`` /
    ``best.ckpt``), ``model_state_dict``, or ``raw`` (a bare state dict: ``vit-mae.pt``)."""
    if not isinstance(ckpt, dict):
        raise ValueError(f"a checkpoint must be a dict, got {type(ckpt).__name__}")
    if "state_dict" in ckpt:
        state, layout = ckpt["state_dict"], "state_dict"
    elif "model_state_dict" in ckpt:
        state, layout = ckpt["model_state_dict"], "model_state_dict"
    else:
        state, layout = ckpt, "raw"
    if not isinstance(state, dict) or not all(isinstance(k, str) and isinstance(v, torch.Tensor) for k, v in state.items()) or not state:
        raise ValueError(f"checkpoint layout {layout!r}: expected a non-empty dict of name -> tensor")
    return {k[len("model."):] if k.startswith("model.") else k: v for k, v in state.items()}, layout


def checkpoint_norm_pix_loss(ckpt: Any) -> Optional[bool]:
    """The ``norm_pix_loss`` flag a checkpoint was trained with (``hyper_parameters.model_cfg.general``, where
    ``MAEPretrainModule.checkpoint_dict`` puts the model config), or None when the checkpoint does not record one."""
    try:
        general = ckpt["hyper_parameters"]["model_cfg"]["general"]
    except (KeyError, TypeError):
        return None
    if not isinstance(general, dict) or "norm_pix_loss" not in general:
        return None
    return bool(general["norm_pix_loss"])


def load_mae_checkpoint(src: Union[str, Path, Dict[str, Any]], model_cfg: Dict[str, Any],
                        precision: Optional[str] = None) -> Tuple[MaskedAutoencoder, str]:
    """A ``MaskedAutoencoder`` built from ``model_cfg`` (the ``model`` section of a config: general / encoder / decoder) with
    the weights of ``src`` (a path or a loaded checkpoint), and the name of the layout found (``mae_state_dict``).
    Unlike the reference's ``load_state_dict(strict=False)`` (:119) a missing or an unexpected tensor raises: a model that
    silently kept its random decoder would still draw a figure.
    ``norm_pix_loss``: a Lightning-layout checkpoint records the flag it was trained with (``checkpoint_norm_pix_loss``); when
    ``model_cfg`` does not set the key the recorded value is used (one line is printed), when both are there and differ the
    call raises.  A bare state dict carries no flag: ``model_cfg`` decides."""
    general = dict(model_cfg.get("general", {}))
    if precision is not None:
        general["engine_precision"] = precision
    if isinstance(src, (str, Path)):
        if not Path(src).exists():
            raise FileNotFoundError(f"Checkpoint not found at {src}")
        src = torch.load(src, map_location="cpu", weights_only=True)
    recorded = checkpoint_norm_pix_loss(src)
    if recorded is not None:
        if "norm_pix_loss" not in general:
            general["norm_pix_loss"] = recorded
            print(f"norm_pix_loss = {recorded} (taken from the checkpoint's hyper_parameters; the config does not set it)")
        elif bool(general["norm_pix_loss"]) != recorded:
            raise ValueError(f"norm_pix_loss: the config says {bool(general['norm_pix_loss'])} but the checkpoint was trained with {recorded}; "
                             "a prediction made in one target space cannot be read in the other")
    model = MaskedAutoencoder(general, model_cfg.get("encoder", {}), model_cfg.get("decoder", {}))
    state, layout = mae_state_dict(src)
    expected = list(model.state_dict().keys())
    missing = [k for k in expected if k not in state]
    unexpected = [k for k in state if k not in set(expected)]
    if missing or unexpected:
        raise ValueError(f"checkpoint (layout {layout!r}) does not match the model: missing {missing[:5]}{' ...' if len(missing) > 5 else ''}, "
                         f"unexpected {unexpected[:5]}{' ...' if len(unexpected) > 5 else ''}")
    model.load_state_dict(state, strict=True)
    return model, layout


# ---------------------------------------------------------------------------------------------------------------------
# statistics
# ---------------------------------------------------------------------------------------------------------------------
def reconstruction_stats(sum_sq, sum_abs, pixels_per_image: int, masked_pixels_per_image: int) -> Dict[str, float]:
    """MSE / L1 / PSNR of ``_print_reconstruction_stats`` (:324-334) from per-image sums, in float64 on the host:
    ``mse`` = nn.MSELoss()(original, reconstructed) and ``l1`` = nn.L1Loss() over every pixel of every image,
    ``psnr`` = -10 log10(mse) (the reference's formula as it stands: no peak term), ``masked_mse`` = the same squared error
    over the masked pixels only, i.e. the validation loss at that mask."""
    sq = torch.as_tensor(sum_sq).detach().to("cpu", torch.float64).reshape(-1)
    ab = torch.as_tensor(sum_abs).detach().to("cpu", torch.float64).reshape(-1)
    if sq.numel() != ab.numel() or sq.numel() == 0:
        raise ValueError(f"sum_sq and sum_abs must hold one entry per image, got {sq.numel()} and {ab.numel()}")
    if pixels_per_image < 1 or not 1 <= masked_pixels_per_image <= pixels_per_image:
        raise ValueError(f"bad pixel counts ({pixels_per_image}, {masked_pixels_per_image})")
    n = sq.numel()
    mse = float(sq.sum()) / (n * pixels_per_image)
    return dict(images=n, mse=mse, l1=float(ab.sum()) / (n * pixels_per_image),
                psnr=-10.0 * math.log10(mse) if mse > 0 else float("inf"),
                masked_mse=float(sq.sum()) / (n * masked_pixels_per_image))


def _pixel_counts(model: MaskedAutoencoder, mask_ratio: Optional[float]) -> Tuple[int, int]:
    m = model.sequence_length - model.num_keep(mask_ratio)
    return model.in_chans * model.image_size ** 2, m * model.patch_dim


def _images_of(batch) -> torch.Tensor:
    if isinstance(batch, (list, tuple)):
        return batch[0]
    return getattr(batch, "images", batch)  # ShardedBatch


def _iterate(batches) -> Iterable:
    return batches() if callable(batches) else batches


def fixed_noise(batch: int, seq_len: int, gen: torch.Generator) -> torch.Tensor:
    return torch.rand(batch, seq_len, generator=gen)


@torch.no_grad()
def evaluate_reconstruction(model: MaskedAutoencoder, batches, mask_ratio: Optional[float] = None, mask_seed: int = MASK_SEED) -> Dict[str, float]:
    """``reconstruction_stats`` over a whole split: ``batches`` yields image batches (uint8 go straight into the engine) or
    (images, labels) pairs, or is a callable returning such an iterator.  The masks come from ONE CPU generator seeded with
    ``mask_seed`` that runs on through the batches.  The per-image sums stay on the device: one host sync, at the end."""
    gen = torch.Generator().manual_seed(int(mask_seed))
    sq, ab = [], []
    for batch in _iterate(batches):
        images = _images_of(batch)
        if images.shape[0] == 0:
            continue
        r = model.reconstruct(images, noise=fixed_noise(images.shape[0], model.sequence_length, gen), mask_ratio=mask_ratio, out="uint8")
        sq.append(r.sum_sq)
        ab.append(r.sum_abs)
    if not sq:
        raise ValueError("evaluate_reconstruction: the split is empty")
    return reconstruction_stats(torch.cat(sq), torch.cat(ab), *_pixel_counts(model, mask_ratio))


# ---------------------------------------------------------------------------------------------------------------------
# figure
# ---------------------------------------------------------------------------------------------------------------------
def to_display_u8(x: torch.Tensor) -> torch.Tensor:
    """``_tensor_to_image`` (:311-322) then ``mul(255).round()``: normalised fp32 -> display uint8 (uint8 passes through)."""
    if x.dtype == torch.uint8:
        return x
    return (x.float() * 0.5 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8)


def save_reconstruction_figure(original_u8, masked_u8, recon_u8, path, mask_ratio: float = 0.75) -> Path:
    """The reference's 3 x n grid (``_visualize_reconstruction``, :273-309): rows "Original", "Masked (75%)", "Reconstructed",
    from three (n, C, H, W) uint8 arrays (torch or numpy; C = 1 or 3)."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np

    rows = []
    for a in (original_u8, masked_u8, recon_u8):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.ndim != 4 or a.dtype != np.uint8:
            raise ValueError(f"expected (n, C, H, W) uint8 arrays, got {a.shape} {a.dtype}")
        rows.append(a.transpose(0, 2, 3, 1))
    n = rows[0].shape[0]
    if n < 1 or any(r.shape != rows[0].shape for r in rows):
        raise ValueError("the three arrays must have the same non-empty shape")
    fig, axes = plt.subplots(3, n, figsize=(2 * n, 6))
    axes = np.asarray(axes).reshape(3, n)
    titles = ("Original", f"Masked ({mask_ratio:.0%})", "Reconstructed")
    for r in range(3):
        for i in range(n):
            img = rows[r][i]
            axes[r, i].imshow(img[..., 0] if img.shape[-1] == 1 else img, cmap="gray" if img.shape[-1] == 1 else None, vmin=0, vmax=255)
            axes[r, i].set_title(titles[r])
            axes[r, i].axis("off")
    plt.tight_layout()
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    fig.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    return path


# ---------------------------------------------------------------------------------------------------------------------
# the reference's class
# ---------------------------------------------------------------------------------------------------------------------
class MAEReconstructor:
    """Handles MAE model reconstruction and validation: the reference's surface (``__init__``, ``load_model``,
    ``reconstruct_batch``, ``validate_reconstruction``).

    The mask is fixed, as in the reference: every call draws ``torch.rand(B, L, generator=torch.Generator().manual_seed(
    mask_seed))`` on the CPU (mask_seed 42) and ranks it as ``random_token_mask`` does.  It is NOT lightly's draw on the
    device after ``torch.manual_seed(42)``, so the masked patches differ from those of the reference's figure.
    ``model_path`` "random" keeps the seeded random initialisation (the chance baseline)."""

    def __init__(self, model_path: str, device: Optional[str] = None, mask_ratio: float = 0.75, mask_seed: int = MASK_SEED,
                 precision: Optional[str] = None):
        self.model_path = model_path if str(model_path) == "random" else Path(model_path)
        if device is None and not torch.cuda.is_available():
            raise RuntimeError("MAEReconstructor: the MI355X engine has no CPU fallback")
        self.device = torch.device(device or "cuda")
        self.mask_ratio = mask_ratio
        self.mask_seed = int(mask_seed)
        self.precision = precision
        self.model: Optional[MaskedAutoencoder] = None
        self.layout: Optional[str] = None
        self.stats: Optional[Dict[str, float]] = None

    def load_model(self, general_cfg: Dict[str, Any], encoder_cfg: Dict[str, Any], decoder_cfg: Dict[str, Any]) -> None:
        model_cfg = dict(general=general_cfg, encoder=encoder_cfg, decoder=decoder_cfg)
        if str(self.model_path) == "random":
            general = dict(general_cfg, **({"engine_precision": self.precision} if self.precision is not None else {}))
            self.model, self.layout = MaskedAutoencoder(general, encoder_cfg, decoder_cfg), "random"
            self.model._init_weights(seed=73)
        else:
            self.model, self.layout = load_mae_checkpoint(self.model_path, model_cfg, precision=self.precision)
            print(f"Model loaded successfully from {self.model_path} (layout: {self.layout})")
        self.model.mask_ratio = self.mask_ratio
        self.model.to(self.device)
        self.model.eval()

    def _run(self, images: torch.Tensor, out: str):
        if self.model is None:
            raise RuntimeError("Model not loaded. Call load_model() first.")
        noise = fixed_noise(images.shape[0], self.model.sequence_length, torch.Generator().manual_seed(self.mask_seed))
        return self.model.reconstruct(images.to(self.device), noise=noise, mask_ratio=self.mask_ratio, out=out)

    def reconstruct_batch(self, images: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(original, masked, reconstructed), each (B, C, H, W) normalised fp32 on the device; images uint8 or normalised."""
        r = self._run(images, "float")
        images = images.to(self.device)
        return (normalize_u8(images) if images.dtype == torch.uint8 else images.float()), r.masked, r.reconstructed

    def validate_reconstruction(self, dataloader, num_samples: int = 8, save_path: Optional[str] = None) -> Dict[str, float]:
        """The first ``num_samples`` images of the first batch: figure (when ``save_path``), the statistics block, and the
        statistics as a dict (also kept in ``self.stats``)."""
        images = _images_of(next(iter(_iterate(dataloader))))[:num_samples]
        r = self._run(images, "uint8")
        if save_path:
            save_reconstruction_figure(to_display_u8(images), r.masked, r.reconstructed, save_path, self.mask_ratio)
            print(f"Visualization saved to {save_path}")
        self.stats = reconstruction_stats(r.sum_sq, r.sum_abs, *_pixel_counts(self.model, self.mask_ratio))
        print_reconstruction_stats(self.stats)
        return self.stats


def print_reconstruction_stats(stats: Dict[str, float]) -> None:
    """The reference's three-line block (``_print_reconstruction_stats``, :331-334)."""
    print("\nReconstruction Statistics:")
    print(f"MSE Loss: {stats['mse']:.6f}")
    print(f"MAE Loss: {stats['l1']:.6f}")
    print(f"PSNR: {stats['psnr']:.2f} dB")
