"""float64 reference of the normalised-pixel targets (norm_pix_loss) for the tests: the oracle's target (``build_target``:
patchify + gather, per-patch order (py, px, c)) standardised per row with ``torch.var(..., unbiased=True)`` and eps 1e-6, as the
MAE code does.  Inputs are taken as the kernels see them: uint8 images after ToTensor + Normalize(.5, .5) in fp32."""
import types

import torch

from oracle import mae_oracle as O

EPS = 1e-6


def normalize_u8(x: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize(.5, .5) as torch computes it in fp32 (uint8 in); fp32 passes through."""
    return (x.to(torch.float32) / 255.0 - 0.5) / 0.5 if x.dtype == torch.uint8 else x.to(torch.float32)


def patches_ref(images: torch.Tensor, idx_mask: torch.Tensor, patch_size: int) -> torch.Tensor:
    """(B, m, P) float64: the fp32 pixel values of patch idx_mask[b][j] - 1, exactly."""
    x = normalize_u8(images.cpu()).double()
    return O.build_target(x, idx_mask.cpu().long(), types.SimpleNamespace(patch_size=int(patch_size)))


def standardise(x: torch.Tensor):
    """(t, mean, rstd) of rows x (..., P) in float64: t = (x - mean) / sqrt(var_unbiased + EPS)."""
    x = x.double()
    mean = x.mean(dim=-1, keepdim=True)
    var = torch.var(x, dim=-1, unbiased=True, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    return (x - mean) * rstd, mean.squeeze(-1), rstd.squeeze(-1)


def target_ref(images: torch.Tensor, idx_mask: torch.Tensor, patch_size: int):
    """(t, mean, rstd) float64 of the masked patches: t (B, m, P), mean / rstd (B, m)."""
    return standardise(patches_ref(images, idx_mask, patch_size))


def loss_ref(pred: torch.Tensor, images: torch.Tensor, idx_mask: torch.Tensor, patch_size: int, grad_scale: float = 1.0):
    """(loss, d_pred) float64: mean((pred - t)^2) over every element and grad_scale * 2 * (pred - t) / n."""
    t, _mean, _rstd = target_ref(images, idx_mask, patch_size)
    d = pred.detach().cpu().double() - t
    return float((d * d).mean()), d * (2.0 * grad_scale / d.numel())


def bound(t: torch.Tensor, rstd: torch.Tensor) -> torch.Tensor:
    """Per-element error bound of an fp32 target: 2^-20 * (rstd_row + |t|).  Inputs lie in [-1, 1]; the centred value carries at
    most ~16 fp32 roundings of 2^-24 (lane-strided partial sums, a 6-step wave reduction, the subtraction), which rstd then
    multiplies; rstd itself is good to a few ulps, relative."""
    return 2.0 ** -20 * (rstd.unsqueeze(-1) + t.abs())
