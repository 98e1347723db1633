"""numpy restatement of mae_augment_ops_u8 (k_augment.hip): every op with PIL's semantics per element, the crop map, the erase
noise and the output conversion.  tests/test_augment_host.py holds this file against Pillow bit for bit; the GPU test holds the
kernel against this file, exactly equal for the bytes and within NOISE_TOL for the erase noise.

Images are (C, S, S) uint8 arrays.  An op chain feeds every op the rounded uint8 result of the op before it, as a chain of PIL
transforms does.  Integer ops are integers here, the blends are fp32 and the lookup tables / the affine map are fp64, each
operation rounded on its own (numpy never fuses a multiply with an add), which is the order Pillow's C code has on a
baseline x86-64 build.

Erase noise.  Element e = (c S + y) S + x of an image with seed s gets
  w0 = mix(s, 2e), w1 = mix(s, 2e + 1),   mix(s, i) = fmix32(fmix32(i + 0x9E3779B9) ^ s)   (murmur3's finaliser),
  u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1],  u2 = (w1 >> 8) 2^-24 in [0, 1),  n = sqrt(-2 ln u1) cos(2 pi u2).
The reference evaluates n in fp64 from the same integers; the kernel in fp32 with logf / sqrtf / cosf.  Bound on the difference:
  radius r = sqrt(-2 ln u1) <= sqrt(2 * 24 ln 2) = 5.77;
  u1, u2 are exact in fp32 (24-bit integers times 2^-24);
  logf is good to 1 ulp (HIP's documented bound) and -2 ln u1 is at most 33.3, sqrtf to 1 ulp: the relative error of r is at
    most (1/2) 2^-23 (log, halved by the root; where ln u1 is near 0 its absolute error 2^-24 * |ln u1| keeps the same
    relative size) + 2^-23 (sqrt) < 1.8e-7, so |dr| <= 5.77 * 1.8e-7 = 1.1e-6;
  the argument fl(2 pi) * u2 < 6.29: rounding the product costs at most 2^-22 = 2.4e-7 (half an ulp at 4..8), fl(2 pi)
    differs from 2 pi by 1.75e-7, times u2 < 1: |darg| <= 4.2e-7, and |d cos| <= |darg|;
  cosf is good to 2 ulp of a value <= 1: 2.4e-7.
  |dn| <= |dr| * 1 + r * (4.2e-7 + 2.4e-7) <= 1.1e-6 + 5.77 * 6.6e-7 = 4.9e-6  <  1e-5.
NOISE_TOL = 2e-5 absolute leaves a factor of four over that.
"""
from __future__ import annotations

import math

import numpy as np

NONE, AUTOCONTRAST, EQUALIZE, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, COLOR, CONTRAST, BRIGHTNESS, SHARPNESS, AFFINE = range(12)
COLOUR_OPS = (COLOR, CONTRAST)   # the ops that read a luminance: three channels only
BILINEAR, BICUBIC, BILINEAR_ROUND, BICUBIC_ROUND = 0, 1, 2, 3
NOISE_TOL = 2e-5


# ---- point ops ---------------------------------------------------------------------------------------------------------
def invert(img):
    return (255 - img.astype(np.int32)).astype(np.uint8)


def solarize(img, t):
    v = img.astype(np.int32)
    return np.where(v < t, v, 255 - v).astype(np.uint8)


def solarize_add(img, a):
    v = img.astype(np.int32)
    return np.where(v < 128, np.clip(v + a, 0, 255), v).astype(np.uint8)


def posterize(img, bits):
    if bits >= 8:
        return img.copy()
    if bits <= 0:
        return np.zeros_like(img)
    return (img & np.uint8(~((1 << (8 - bits)) - 1) & 0xff)).astype(np.uint8)


def autocontrast_lut(h):
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    i = np.arange(256, dtype=np.float64)
    return np.clip((i * scale + off).astype(np.int64), 0, 255).astype(np.uint8)   # astype truncates toward zero like int()


def equalize_lut(h):
    h = h.astype(np.int64)
    nz = h[h > 0]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return ident
    step = int(nz.sum() - nz[-1]) // 255
    if step == 0:
        return ident
    before = np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(255, (step // 2 + before) // step).astype(np.uint8)


def _per_channel_lut(img, make):
    out = np.empty_like(img)
    for c in range(img.shape[0]):
        out[c] = make(np.bincount(img[c].reshape(-1), minlength=256))[img[c]]
    return out


def autocontrast(img):
    return _per_channel_lut(img, autocontrast_lut)


def equalize(img):
    return _per_channel_lut(img, equalize_lut)


# ---- blends ------------------------------------------------------------------------------------------------------------
def luminance(img):
    r, g, b = (img[c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.int32)


def blend(d, v, f):
    """Image.blend(degenerate, image, f) per element: fp32, the product and the sum rounded separately."""
    alpha = np.float32(f)
    d = np.broadcast_to(np.asarray(d, dtype=np.int32), v.shape)
    t = d.astype(np.float32) + alpha * (v.astype(np.int32) - d).astype(np.float32)
    if 0.0 <= float(alpha) <= 1.0:
        return np.trunc(t).astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.int32).astype(np.uint8)


def color(img, f):
    return blend(luminance(img)[None], img, f)


def contrast(img, f):
    S2 = img.shape[1] * img.shape[2]
    mean = int(int(luminance(img).sum()) / float(S2) + 0.5)
    return blend(mean, img, f)


def brightness(img, f):
    return blend(0, img, f)


def smooth(img):
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 rounded to nearest; the one-pixel border is the source pixel."""
    v = img.astype(np.int64)
    out = v.copy()
    s = 4 * v[:, 1:-1, 1:-1]
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            s = s + v[:, dy:v.shape[1] - 2 + dy, dx:v.shape[2] - 2 + dx]
    if s.size:
        out[:, 1:-1, 1:-1] = (2 * s + 13) // 26
    return out.astype(np.int32)


def sharpness(img, f):
    return blend(smooth(img), img, f)


# ---- affine ------------------------------------------------------------------------------------------------------------
def _bicubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, m, mode=BICUBIC, fill=0):
    """Image.transform(size, AFFINE, m, resample, fillcolor) in fp64; ``fill`` is 0xRRGGBB (channel c takes byte 2 - c; a
    one-channel image the low byte).  Modes 2 / 3 round to nearest instead of truncating (the crop's modes)."""
    C, S, _ = img.shape
    m = [float(x) for x in m]
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64) + 0.5, np.arange(S, dtype=np.float64) + 0.5, indexing="ij")
    xin = m[0] * xx + m[1] * yy + m[2]
    yin = m[3] * xx + m[4] * yy + m[5]
    outside = ~((xin >= 0.0) & (xin < S) & (yin >= 0.0) & (yin < S))   # PIL's test; a NaN coordinate counts as outside
    xin = np.where(outside, 0.5, xin) - 0.5
    yin = np.where(outside, 0.5, yin) - 0.5
    x = np.floor(xin).astype(np.int64)
    y = np.floor(yin).astype(np.int64)
    dx, dy = xin - x, yin - y
    cl = lambda i: np.clip(i, 0, S - 1)
    out = np.empty_like(img)
    for c in range(C):
        p = img[c].astype(np.float64)
        if mode in (BILINEAR, BILINEAR_ROUND):
            x0, x1 = cl(x), cl(x + 1)
            r = []
            for yi in (cl(y), cl(y + 1)):
                a, b = p[yi, x0], p[yi, x1]
                r.append(a + (b - a) * dx)
            v = r[0] + (r[1] - r[0]) * dy
        else:
            xs = [cl(x - 1), cl(x), cl(x + 1), cl(x + 2)]
            r = [_bicubic(*(p[cl(y + k), xi] for xi in xs), dx) for k in (-1, 0, 1, 2)]
            v = _bicubic(*r, dy)
        if mode == BILINEAR:
            q = np.trunc(v)
        elif mode == BICUBIC:
            q = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, np.trunc(v)))
        else:
            q = np.where(v <= 0.0, 0.0, np.where(v >= 255.0, 255.0, np.floor(v + 0.5)))
        fc = (fill >> (8 * (2 - c))) & 0xff if C == 3 else fill & 0xff
        out[c] = np.where(outside, fc, q).astype(np.int64).astype(np.uint8)
    return out


def crop_matrix(top, left, h, w, flip, S):
    """The random-resized crop (+ flip) as an affine map of output pixel centres into the box: always inside the image."""
    if flip:
        return (-w / S, 0.0, float(left + w), 0.0, h / S, float(top))
    return (w / S, 0.0, float(left), 0.0, h / S, float(top))


def rotate_matrix(deg, S):
    """The matrix Image.rotate(deg) hands to transform(AFFINE): cos / sin of -radians(deg) rounded to 15 places, about (S/2, S/2)."""
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx = cy = S / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


# ---- the chain ---------------------------------------------------------------------------------------------------------
def apply_op(img, code, iarg, args):
    C = img.shape[0]
    if code in COLOUR_OPS and C != 3:
        return img
    f = float(args[0])
    if code == AUTOCONTRAST: return autocontrast(img)
    if code == EQUALIZE: return equalize(img)
    if code == INVERT: return invert(img)
    if code == POSTERIZE: return posterize(img, int(iarg))
    if code == SOLARIZE: return solarize(img, int(iarg))
    if code == SOLARIZE_ADD: return solarize_add(img, int(iarg))
    if code == COLOR: return color(img, f)
    if code == CONTRAST: return contrast(img, f)
    if code == BRIGHTNESS: return brightness(img, f)
    if code == SHARPNESS: return sharpness(img, f)
    if code == AFFINE: return affine(img, args, int(iarg) & 0xff, (int(iarg) >> 8) & 0xffffff)
    return img   # NONE and every unknown id


def apply_ops(images, op_codes, op_args):
    """(B, C, S, S) uint8 through (B, K, 2) int32 codes and (B, K, 6) fp64 arguments, slot by slot."""
    out = np.empty_like(images)
    for b in range(images.shape[0]):
        img = images[b]
        for k in range(op_codes.shape[1]):
            img = apply_op(img, int(op_codes[b, k, 0]), int(op_codes[b, k, 1]), op_args[b, k])
        out[b] = img
    return out


# ---- erase noise and output --------------------------------------------------------------------------------------------
def normalize_u8_f32(x):
    v = x.astype(np.float32) / np.float32(255.0)
    return (v - np.float32(0.5)) / np.float32(0.5)


def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xffffffff
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xffffffff
    h ^= h >> 16
    return h


def _mix(seed, i):
    return _fmix32(_fmix32((i + 0x9E3779B9) & 0xffffffff) ^ np.uint64(seed & 0xffffffff))


def erase_noise(C, S, seed):
    """(C, S, S) fp64 N(0, 1) noise of one image."""
    e = np.arange(C * S * S, dtype=np.uint64).reshape(C, S, S)
    w0, w1 = _mix(int(seed), (2 * e) & 0xffffffff), _mix(int(seed), (2 * e + 1) & 0xffffffff)
    u1 = ((w0 >> 8) + 1).astype(np.float64) * 2.0 ** -24
    u2 = (w1 >> 8).astype(np.float64) * 2.0 ** -24
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def erase_mask(erase, S):
    """(B, S, S) bool from (B, 5) rows (y0, y1, x0, x1, seed): half-open, clamped to [0, S]; empty / inverted boxes erase nothing."""
    bx = np.clip(np.asarray(erase, dtype=np.int64)[:, :4], 0, S)
    yy, xx = np.arange(S)[None, :, None], np.arange(S)[None, None, :]
    return (yy >= bx[:, 0, None, None]) & (yy < bx[:, 1, None, None]) & (xx >= bx[:, 2, None, None]) & (xx < bx[:, 3, None, None])


def output_f32(images_u8, erase=None):
    """MAE_F32 output: (fp32 normalised bytes, bool mask of the erased elements, fp64 noise where the mask is set)."""
    B, C, S, _ = images_u8.shape
    base = normalize_u8_f32(images_u8)
    mask = np.zeros(images_u8.shape, dtype=bool)
    noise = np.zeros(images_u8.shape, dtype=np.float64)
    if erase is not None:
        mask = np.broadcast_to(erase_mask(erase, S)[:, None], images_u8.shape).copy()
        for b in range(B):
            if mask[b].any():
                noise[b] = erase_noise(C, S, int(erase[b][4]))
    return base, mask, noise


# ---- the test images (host and GPU tests share them) ---------------------------------------------------------------------
def sample_images(C, S, seed=0):
    """name -> (C, S, S) uint8: noise, a 40..199 narrow-range image, a ramp and a constant image."""
    g = np.random.default_rng(1000 * seed + 10 * S + C)
    noise = g.integers(0, 256, (C, S, S), dtype=np.uint8)
    noise.reshape(-1)[:2] = (0, 255)
    narrow = g.integers(40, 200, (C, S, S), dtype=np.uint8)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    ramp = np.stack([((xx * 255) // max(S - 1, 1)), ((yy * 255) // max(S - 1, 1)), (((xx + yy) * 255) // max(2 * S - 2, 1))][:C]).astype(np.uint8)
    const = np.full((C, S, S), 77, dtype=np.uint8)
    return {"noise": noise, "narrow": narrow, "ramp": ramp, "const": const}
