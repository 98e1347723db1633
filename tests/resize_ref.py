"""float64 reference of mae_resize_crop_flip (k_resize.hip), its error bound, and an fp32 restatement of the kernel's arithmetic.

Definition (include/mae_hip.h).  Image b of (B, C, Si, Si) goes to (So, So) through its box (top, left, h, w) and flip flag
(no params: the whole image, not flipped).  Per axis (x shown; ox' = So - 1 - ox under a flip), s = w / So and
  c = left + w (2 ox' + 1) / (2 So) - 0.5
  w <= So: c clamped to [0, Si - 1]; taps floor(c) and min(floor(c) + 1, Si - 1), weights (1 - a, a), a = c - floor(c)
  w >  So: taps j = ceil(c - s) .. floor(c + s), those outside [0, Si - 1] dropped, weight max(0, 1 - |j - c| / s) divided by
           the sum of the kept weights.
The pixel is the separable sum  sum_jy Wy[oy][jy] sum_jx Wx[ox][jx] p[jy][jx].  ``resize_reference`` evaluates it in fp64
from one dense (So, Si) weight matrix per axis and image.

Bound.  u = 2^-24, P = the largest |pixel| of the image (255 for bytes), SECOND = 1 + 2^-16 for the second-order terms (the
convention of tests/optim_ref.py).  The kernel holds the coordinate in integers (D = 2 So, N = w (2 ox' + 1) - So,
c = left + N / D), so the fp32 coordinate costs nothing before the weight: tap j weighs 1 - |D (j - left) - N| / G with
G = max(2 w, 2 So), evaluated as 1 - float(|m|) * fl(1 / G): the integer is exact (< 2^24), the reciprocal and the product
round a number <= 1 (2 u), the subtraction rounds a number <= 1 (u): every raw weight is within 3 u.  Per axis, with n kept
taps whose raw weights sum to S (S = 1 where the axis does not shrink):
  raw weights           3 u each:                         the normalised sum moves by <= 3 n / S u P
  accumulation          n products and n sums, unfused:   <= 2 n u P   (the library fuses them: that only removes roundings)
  1 / S                 S itself is off by 3 n u + (n - 1) u S, the reciprocal rounds once: relative <= (3 n / S + n) u
so an axis contributes E(n, S) = (6 n / S + 3 n) u P, and the pixel
  delta = (E(nx, Sx) + E(ny, Sy) + 3 u P) SECOND        (3: the product of the two 1 / S, the scaling, one spare)
n and S are read off the fp64 weight matrices, never off the kernel's output.  For bytes delta is about 6e-4 grey levels where
both axes take two taps and 2e-3 at 17 taps an axis: above the 1e-4 an fp32 evaluation of these sums reaches on the host,
below the 1e-2 that the same-size crop test allows.  uint8 output rounds to nearest: |out - ref| <= 0.5 + delta; fp32
output of fp32 images: delta; fp32 output of bytes is normalize_u8 of the uint8 output, bit for bit.

``resize_emulated_f32`` restates the kernel in numpy fp32, one rounding per operation (unfused), taps in ascending order.
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -16

# (B, C, Si, So): non-integer / integer upsample, integer / non-integer downsample, a small odd output, the two store tails
# (So % 4 = 2 and 1, rows off the 4-byte grid), the workload's own size, the same size
CASES = [(3, 3, 96, 112), (2, 1, 32, 64), (2, 3, 96, 32), (2, 3, 96, 40), (2, 4, 12, 7), (1, 3, 8, 18), (1, 3, 8, 21), (5, 3, 96, 224),
         (4, 3, 96, 96)]


def whole(B: int, Si: int, flip: int = 0) -> np.ndarray:
    return np.tile(np.array([[0, 0, Si, Si, flip]], dtype=np.int32), (B, 1))


def box_sets(B: int, Si: int, seed: int = 0):
    """[(name, (B, 5) int32)]: the whole image, flips, 1 x 1 boxes, boxes on each border, full-height one-column and full-width
    one-row boxes (one axis grows while the other shrinks or stays), and seeded RandomResizedCrop draws at two scales."""
    import torch
    from ssrl_vit_mae_jepa_amd.data import random_resized_crop_params
    sets = [("whole", whole(B, Si)), ("flip", whole(B, Si, 1))]
    spots = [(0, 0), (Si - 1, Si - 1), (Si // 2, 1), (0, Si - 1), (Si - 1, Si // 3)]
    sets.append(("1x1", np.array([[*spots[b % 5], 1, 1, b & 1] for b in range(B)], dtype=np.int32)))
    hh, ww = max(1, (2 * Si) // 3), max(1, Si // 2)
    edges = [(0, min(3, Si - ww), hh, ww), (Si - hh, min(2, Si - ww), hh, ww), (min(1, Si - ww), 0, ww, hh), (min(2, Si - ww), Si - hh, ww, hh),
             (Si - 1, 0, 1, Si)]
    for k in range(0, len(edges), B):  # every border reaches every shape
        rows = [edges[(k + b) % len(edges)] for b in range(B)]
        sets.append((f"borders{k}", np.array([[*r, (b + k) & 1] for b, r in enumerate(rows)], dtype=np.int32)))
    sets.append(("column", np.array([[0, (b * 5) % Si, Si, 1, b & 1] for b in range(B)], dtype=np.int32)))
    sets.append(("row", np.array([[(b * 7 + 1) % Si, 0, 1, Si, b & 1] for b in range(B)], dtype=np.int32)))
    for name, scale in (("rrc08", (0.08, 1.0)), ("rrc80", (0.8, 1.0))):
        g = torch.Generator().manual_seed(1000 * seed + Si + B)
        top, left, h, w = random_resized_crop_params(B, Si, g, scale=scale)
        flip = (torch.rand(B, generator=g) < 0.5).to(torch.int64)
        sets.append((name, torch.stack([top, left, h, w, flip], dim=1).numpy().astype(np.int32)))
    return sets


def axis_matrix(So: int, Si: int, start: int, length: int, flip: bool):
    """One axis of one image: (W (So, Si) fp64 normalised weights, n (So) kept taps of positive weight, S (So) their raw sum)."""
    o = np.arange(So)
    om = So - 1 - o if flip else o
    s = length / So
    c = start + length * (2 * om + 1) / (2.0 * So) - 0.5
    W = np.zeros((So, Si), dtype=np.float64)
    if length <= So:
        cc = np.clip(c, 0.0, Si - 1.0)
        j0 = np.floor(cc).astype(np.int64)
        a = cc - j0
        np.add.at(W, (o, j0), 1.0 - a)
        np.add.at(W, (o, np.minimum(j0 + 1, Si - 1)), a)
        return W, np.where(a > 0, 2, 1), np.ones(So)
    j = np.arange(Si)[None, :]
    keep = (j >= np.ceil(c - s)[:, None]) & (j <= np.floor(c + s)[:, None])
    w = np.where(keep, np.maximum(0.0, 1.0 - np.abs(j - c[:, None]) / s), 0.0)
    S = w.sum(axis=1)
    return w / S[:, None], (w > 0).sum(axis=1), S


def axis_error(n: np.ndarray, S: np.ndarray) -> np.ndarray:
    """E(n, S) / (u P) of the module docstring."""
    return 6.0 * n / S + 3.0 * n


def resize_reference(images: np.ndarray, params, So: int):
    """(ref fp64 (B, C, So, So), delta fp64 (B, 1, So, So)).  ``images`` uint8 or fp32; params (B, 5) or None."""
    B, C, Si, _ = images.shape
    p = whole(B, Si) if params is None else np.asarray(params)
    x = images.astype(np.float64)
    ref = np.empty((B, C, So, So), dtype=np.float64)
    delta = np.empty((B, 1, So, So), dtype=np.float64)
    for b in range(B):
        top, left, h, w, flip = (int(v) for v in p[b])
        Wy, ny, Sy = axis_matrix(So, Si, top, h, False)
        Wx, nx, Sx = axis_matrix(So, Si, left, w, bool(flip))
        ref[b] = np.matmul(np.matmul(Wy[None], x[b]), Wx.T[None])
        P = 255.0 if images.dtype == np.uint8 else float(np.abs(x[b]).max())
        delta[b, 0] = (axis_error(ny, Sy)[:, None] + axis_error(nx, Sx)[None, :] + 3.0) * U * P * SECOND
    return ref, delta


def _axis_f32(So: int, Si: int, start: int, length: int, flip: bool):
    """The kernel's taps of one axis: raw fp32 weights (So, Si) and the fp32 scale 1 / sum (So)."""
    f = np.float32
    D, G = 2 * So, 2 * max(length, So)
    inv_g = f(1.0) / f(G)
    W = np.zeros((So, Si), dtype=np.float32)
    scale = np.ones(So, dtype=np.float32)
    weight = lambda m: max(f(1.0) - f(abs(m)) * inv_g, f(0.0))  # noqa: E731
    for o in range(So):
        om = So - 1 - o if flip else o
        N = length * (2 * om + 1) - So
        q = N // D
        if length <= So:
            r = N - q * D
            if 0 <= start + q < Si - 1 and r != 0:
                W[o, start + q], W[o, start + q + 1] = weight(-r), weight(D - r)
            else:
                W[o, min(max(start + q, 0), Si - 1)] = f(1.0)
            continue
        jl, jh = max(start + (N - 2 * length) // D + 1, 0), min(start - (-(N + 2 * length)) // D - 1, Si - 1)
        total = f(0.0)
        for j in range(jl, jh + 1):
            W[o, j] = weight(D * (j - start) - N)
            total = f(total + W[o, j])
        scale[o] = f(1.0) / total
    return W, scale


def resize_emulated_f32(images: np.ndarray, params, So: int) -> np.ndarray:
    """The fp32 sums of the kernel before the output conversion, (B, C, So, So) fp32."""
    B, C, Si, _ = images.shape
    p = whole(B, Si) if params is None else np.asarray(params)
    x = images.astype(np.float32)
    out = np.empty((B, C, So, So), dtype=np.float32)
    for b in range(B):
        top, left, h, w, flip = (int(v) for v in p[b])
        Wy, sy = _axis_f32(So, Si, top, h, False)
        Wx, sx = _axis_f32(So, Si, left, w, bool(flip))
        rows = np.zeros((C, Si, So), dtype=np.float32)       # every source row through the column taps, ascending
        for j in range(Si):
            rows = (rows + Wx[None, None, :, j] * x[b][:, :, j, None]).astype(np.float32)
        acc = np.zeros((C, So, So), dtype=np.float32)
        for j in range(Si):
            acc = (acc + Wy[None, :, j, None] * rows[:, j, None, :]).astype(np.float32)
        out[b] = acc * (sy[:, None] * sx[None, :]).astype(np.float32)[None]
    return out


def round_u8(v: np.ndarray) -> np.ndarray:
    """rintf and the clamp to a byte."""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


_inputs = {}


def inputs(B: int, C: int, Si: int):
    """Seeded (uint8, fp32) images of one shape, made once; both extreme bytes occur."""
    if (B, C, Si) not in _inputs:
        g = np.random.default_rng(B * 1000 + C * 100 + Si)
        u8 = g.integers(0, 256, (B, C, Si, Si), dtype=np.uint8)
        u8.reshape(-1)[:2] = (0, 255)
        f32 = (g.standard_normal((B, C, Si, Si)) * 1.5).astype(np.float32)
        u8.setflags(write=False); f32.setflags(write=False)
        _inputs[(B, C, Si)] = (u8, f32)
    return _inputs[(B, C, Si)]


_refs = {}


def reference(case, name: str, params: np.ndarray, dtype: str):
    """``resize_reference`` of a case's seeded inputs under one box set, computed once and shared by the tests."""
    key = (case, name, dtype)
    if key not in _refs:
        B, C, Si, So = case
        u8, f32 = inputs(B, C, Si)
        _refs[key] = resize_reference(u8 if dtype == "u8" else f32, params, So)
    return _refs[key]
