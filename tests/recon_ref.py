"""CPU reference of the MAE reconstruction compose (mae_reconstruct_compose) for the tests: the reference's
``_create_masked_images`` / ``_reconstruct_full_images`` (scripts/evaluation/visualize_reconstruction.py:170-234) restated with
the oracle's patchify / unpatchify and torch.scatter, the fp64 per-image error sums and the uint8 display expression."""
import torch

from oracle import mae_oracle as O


def normalize_u8(x: torch.Tensor) -> torch.Tensor:
    """ToTensor + Normalize(.5, .5) as torch computes it in fp32 (uint8 in); fp32 passes through."""
    return (x.to(torch.float32) / 255.0 - 0.5) / 0.5 if x.dtype == torch.uint8 else x.to(torch.float32)


def display_u8(x: torch.Tensor) -> torch.Tensor:
    """``_tensor_to_image`` (:311-322) followed by mul(255).round(): the torch fp32 expression."""
    return (x * 0.5 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8)


def compose_ref(images: torch.Tensor, pred: torch.Tensor, idx_mask: torch.Tensor, patch_size: int, fill: float = 0.5):
    """(reconstructed, masked), both (B, C, S, S) normalised fp32: patch n = idx_mask[b][j] - 1 of the normalised image replaced by
    pred[b][j] / by ``fill``.  Entries <= 0 (the class token, ``__remove_cls_token``) or > N are dropped with their pred rows."""
    x = normalize_u8(images.cpu())
    pred, idx_mask = pred.cpu().float(), idx_mask.cpu()
    C = x.shape[1]
    patches = O.patchify(x, patch_size)  # (B, N, P) in (py, px, c) order
    N, P = patches.shape[1], patches.shape[2]
    recon, masked = patches.clone(), patches.clone()
    for b in range(x.shape[0]):
        ok = (idx_mask[b] >= 1) & (idx_mask[b] <= N)
        n = (idx_mask[b][ok] - 1).unsqueeze(-1).expand(-1, P)
        recon[b] = torch.scatter(recon[b], 0, n, pred[b][ok])
        masked[b] = torch.scatter(masked[b], 0, n, torch.full_like(pred[b][ok], fill))
    return O.unpatchify(recon, patch_size, C), O.unpatchify(masked, patch_size, C)


def sums_ref(images: torch.Tensor, recon: torch.Tensor):
    """Per-image (sum d^2, sum |d|) in fp64 of the fp32 terms d = recon - normalised image (visible pixels give exactly 0)."""
    d = recon.cpu().float() - normalize_u8(images.cpu())
    return (d * d).double().flatten(1).sum(1), d.abs().double().flatten(1).sum(1)


def gamma(n: int) -> float:
    """Worst-case relative error of an fp32 sum of n non-negative terms in any order: n u / (1 - n u), u = 2^-24."""
    return n * 2.0 ** -24 / (1.0 - n * 2.0 ** -24)
