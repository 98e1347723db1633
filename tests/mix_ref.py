"""float64 references for the fine-tuning recipe: the soft-target classifier head and the batch mixing kernel (k_mix.hip).

Soft targets.  Row b of a batch with label pair (ya, yb), weight lam and smoothing eps over C classes has the target
  t[b][c] = eps / C + (1 - eps) * (lam[b] [c == ya[b]] + (1 - lam[b]) [c == yb[b]]),       sum_c t = 1,
so row_loss = lse - sum_c t c logit_c and d_logits = (softmax - t) * grad_scale / B.  This is
lam CE(ya, label_smoothing=eps) + (1 - lam) CE(yb, label_smoothing=eps) of torch (tests/test_mix_host.py checks that).
``soft_head_reference`` is tests/test_gpu_classifier.py::head_reference with that target: fp64, with the engine's bf16
rounding points (features as stored, the pooled vector, W, d_logits).  lam enters as the fp32 value the kernel reads.

Mixing.  out = n(partner) inside the box, lam n(own) + (1 - lam) n(partner) outside, where n() is ``normalize_u8`` evaluated
in fp32 for uint8 images (the kernel's normalisation is bit-identical to it: the contract of k_pixels.hip) and the identity
for fp32 images.  The reference mixes those fp32 values in fp64 with lam widened from fp32.
Bound per outside pixel (the convention of tests/optim_ref.py, u = 2^-24, SECOND = 1 + 2^-16 for the second-order terms; the
library is built with -ffp-contract=fast, and fusing only removes roundings):
  fl(1 - lam) = 1, the larger of the two products = 1, the sum = 1          |err| <= 3 u (|lam a| + |(1 - lam) b|) SECOND
Inside-box pixels and pixels with lam == 1 are copies: bit-exact.  uint8 output is a byte select: bit-exact everywhere.
"""
from __future__ import annotations

import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16


def _r(x: torch.Tensor, bf: bool) -> torch.Tensor:
    return x.to(torch.bfloat16).to(torch.float32) if bf else x


def soft_targets(ya, yb, lam, eps: float, C: int) -> torch.Tensor:
    """(B, C) fp64 targets; lam is widened from fp32."""
    lam = torch.as_tensor(lam, dtype=torch.float32).double()[:, None]
    oa = torch.nn.functional.one_hot(ya, C).double()
    ob = torch.nn.functional.one_hot(yb, C).double()
    return eps / C + (1.0 - eps) * (lam * oa + (1.0 - lam) * ob)


def soft_loss(logits: torch.Tensor, ya, yb, lam, eps: float) -> torch.Tensor:
    """Batch-mean soft-target cross-entropy of ``logits`` (any float dtype; differentiable)."""
    t = soft_targets(ya, yb, lam, eps, logits.shape[1]).to(logits.dtype)
    return (torch.logsumexp(logits, dim=1) - (t * logits).sum(dim=1)).mean()


def soft_head_reference(feats, pool: str, lo: int, head, C: int, ya, yb, lam, eps: float, bf: bool, grad_scale: float = 1.0):
    """pool "cls": row 0 (d_feats is (B, D)); "mean": the mean of rows [lo, rows) (d_feats (B, rows, D), zeros below lo).
    Returns logits, loss, correct (argmax == ya), head_grads (dW then db), d_feats -- all fp64."""
    B, rows, D = feats.shape
    x = _r(feats.float(), bf).double()
    pooled = x[:, 0] if pool == "cls" else x[:, lo:].mean(dim=1)
    pooled = _r(pooled.float(), bf).double()
    W = _r(head[:C * D].view(C, D), bf).double()
    b = head[C * D:C * D + C].double()
    logits = pooled @ W.T + b
    t = soft_targets(ya, yb, lam, eps, C)
    loss = (torch.logsumexp(logits, dim=1) - (t * logits).sum(dim=1)).mean()
    dl = (torch.softmax(logits, dim=1) - t) * grad_scale / B
    dl = _r(dl.float(), bf).double()
    dW, db = dl.T @ pooled, dl.sum(0)
    dpool = dl @ W
    if pool == "cls":
        dfeat = dpool
    else:
        dfeat = torch.zeros(B, rows, D, dtype=torch.float64)
        dfeat[:, lo:] = (dpool / (rows - lo))[:, None, :]
    correct = int((logits.argmax(1) == ya).sum())
    return logits, loss, correct, torch.cat([dW.reshape(-1), db]), dfeat


def normalize_u8_f32(x: np.ndarray) -> np.ndarray:
    """``data.normalize_u8`` in numpy fp32: (x / 255 - 0.5) / 0.5, every operation rounded to fp32."""
    v = x.astype(np.float32) / np.float32(255.0)
    return (v - np.float32(0.5)) / np.float32(0.5)


def inside_mask(box: np.ndarray, S: int) -> np.ndarray:
    """(B, S, S) bool: pixel (y, x) of image b lies in its box (y0, y1, x0, x1), half-open, clamped to [0, S]."""
    bx = np.clip(np.asarray(box, dtype=np.int64), 0, S)
    yy, xx = np.arange(S)[None, :, None], np.arange(S)[None, None, :]
    return (yy >= bx[:, 0, None, None]) & (yy < bx[:, 1, None, None]) & (xx >= bx[:, 2, None, None]) & (xx < bx[:, 3, None, None])


def effective_partner(partner: np.ndarray, B: int) -> np.ndarray:
    p = np.asarray(partner, dtype=np.int64)
    return np.where((p < 0) | (p >= B), np.arange(B), p)


def mix_reference(images: np.ndarray, partner, lam, box):
    """fp32 output of mae_mix_batch: (ref fp64, bound fp64, exact bool), each (B, C, S, S).  ``exact`` marks the pixels that
    must match bit for bit (bound 0 there): inside the box, and wherever lam == 1."""
    B, C, S, _ = images.shape
    n = normalize_u8_f32(images) if images.dtype == np.uint8 else images.astype(np.float32)
    a = n.astype(np.float64)
    b = a[effective_partner(partner, B)]
    l = np.asarray(lam, dtype=np.float32).astype(np.float64)[:, None, None, None]
    inside = np.broadcast_to(inside_mask(box, S)[:, None], a.shape)
    ref = np.where(inside, b, l * a + (1.0 - l) * b)
    exact = inside | np.broadcast_to(l == 1.0, a.shape)
    ref = np.where(exact & ~inside, a, ref)
    bound = np.where(exact, 0.0, 3.0 * U * (np.abs(l * a) + np.abs((1.0 - l) * b)) * SECOND)
    return ref, bound, exact


def cutmix_u8_reference(images: np.ndarray, partner, box) -> np.ndarray:
    """uint8 output of mae_mix_batch: the partner's byte inside the box, the own byte outside."""
    B, C, S, _ = images.shape
    inside = np.broadcast_to(inside_mask(box, S)[:, None], images.shape)
    return np.where(inside, images[effective_partner(partner, B)], images)
