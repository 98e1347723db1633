"""numpy restatement of the kernels that move tokens and pixels between the GEMMs, and of the losses that read the image
(k_patch.hip, k_pixels.hip, k_index.hip, k_jepa.hip), for the tests.

numpy on the CPU: no torch, no GPU.  One ``expect_*`` function per kernel family turns a case and its generated inputs into
a dict  output name -> Exact | Bounded | Scratch;  ``judge`` compares what a kernel (or ``simulate``, the plain fp32 numpy
evaluation) left in the output buffers against it and returns ``(worst error / bound per output, failures)``.  Every
output buffer starts from ``init``: NaN-filled (or pattern-filled) with GUARD rows behind it, and the WHOLE buffer is
compared, so a guard row that was written, an untouched row that changed, or a NaN that turned into a number is a failure.

What is exact (compared as integer views, NaN patterns included) and why:
  copies          gather_patches (c, py, px), patchify_gather (py, px, c), dtok, d_xdec of decoder_assemble_bwd: no arithmetic.  The
                  uint8 readers take v = (fl(u / 255) - 0.5) / 0.5 evaluated in np.float32: the division is IEEE-rounded
                  (__fdiv_rn), the subtraction rounds once, the division by 0.5 is exact.
  one fp32 add    assemble_visible, decoder_assemble, predictor_assemble: fl(a + b), which numpy's float32 addition returns.
  bf16 outputs    the round-to-nearest-even of that fp32 value (optim_ref.bf16_rne), a NaN keeps its quiet pattern.
  zeros           zero_unpredicted_rows and the class-token rows of dtok are +0.0; every other row keeps its bits.
  index kernels   integer arithmetic.
  d_pred          fl(fl(pred - t) * gs), then the bf16 rounding.  MSE: gs is the launcher's own fp32 expression
                  grad_scale * 2.0f / (float)n, evaluated left to right.  Smooth-L1: gs = grad_scale / (float)n and the
                  difference is clamped to [-1, 1] first.  The library is built with -ffp-contract=fast, which cannot fuse
                  anything here: no addition follows the product.  (In the uint8 loss the compiler may fold the exact
                  doubling of t into the subtraction; a doubling does not round, so the bits are the same.)
  column sums on the exactness inputs (integers, |x| <= 8, every partial sum below 2^24): every partial sum is an integer
                  that fp32 holds exactly, so any summation order returns the float64 sum.  A dropped or doubled row
                  changes the integer.

The only two bounds, u = 2^-24:
  column sums (dcls, d_mask_token, the mask-token sum and the nblk-fold context sum of predictor_assemble_bwd) on random
  inputs:  |got - ref64| <= c u sum|x| over the summed rows, c = the longest chain of additions one summand goes through:
      split kernels   T + (RPI - 1) + ceil(G / 32) + 32
                      T = ceil(rows / (G RPI)) additions into the thread's accumulator (four rows in flight do not change the
                      count), RPI - 1 in the LDS fold over the block's row offsets (RPI = 256 / (D / 4)), then
                      sum_partials_kernel: ceil(G / 32) per row lane and the 32-row fold; G = min(ceil(rows / RPI), 512).
      context sum     nblk (one accumulator, blocks ascending); a bf16 d_xdec adds its rounding, 2^-8 of the value (8 significant bits).
  Three of the counted additions (the first into each zero accumulator) do not round; they pay for the second-order terms.
  loss scalars (non-negative terms):  |got - ref64| <= (c + 3) u ref64,
      c = A + 6 + 3 + F + 6 + 3:  A additions into the thread's accumulator, the 6 shuffle steps of wave_sum, the 3 adds of
      block_sum_256, then the finalize kernel: F = ceil(grid / 256) per thread, 6 and 3 again.  The 3 on top are the
      subtraction, the square and the inv_n product.
      A:  gather   ceil(rows p p / (256 grid)) C                       grid = min(ceil(rows p p / 256), 1024)
          band     max over blocks of  sum over the block's bands of  ceil(n_band p (p/4) / 256) 4 C
                   (n_band = tokens of the image in that band, counted from the token list), grid = min(B g, 1024)
          smooth-L1 ceil((n / 4) / (256 grid)) 4                       grid = min(ceil(n / 1024), 1024)
Neither bound is fitted to a kernel's output."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests.optim_ref import bf16_rne

U = 2.0 ** -24
GUARD = 8                       # guard rows behind every matrix output
SPLIT_BLOCKS = 512              # visible_grad_split, decoder_assemble_bwd, predictor_assemble_bwd
ROW_BLOCKS = 256 * 16           # decoder_assemble, predictor_assemble, assemble_visible, gather_patches
ZERO_BLOCKS = 8192              # zero_unpredicted_rows
IDX_BLOCKS = 2048               # build_row_map, build_tail_row_map, rows_from_tokens
RED_BLOCKS = 1024               # stage-1 partials of the losses
PARTIAL_BLOCKS = 512            # `partial` holds 512 * D floats (include/mae_hip.h)
SCRATCH_FLOATS = 4096           # loss scratch
INT_FILL = -0x5A5A5A5B          # what integer outputs start from
DIMS = (8, 144, 192, 768, 1024)


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def rpi(D: int) -> int:
    """Rows per block pass of the row kernels: 256 threads, D / 4 per row."""
    return 256 // (D // 4)


def f32(x) -> np.float32:
    return np.float32(x)


# ------------------------------------------------------------------------------------------------ buffers and dtypes
def to_dt(x32: np.ndarray, dtype: str) -> np.ndarray:
    """fp32 values as the buffer of ``dtype`` holds them: float32, or bf16 patterns (uint16)."""
    x32 = np.ascontiguousarray(x32, dtype=np.float32)
    return x32 if dtype == "f32" else bf16_rne(x32)


def from_dt(a: np.ndarray) -> np.ndarray:
    """The fp32 values of a float32 or bf16-pattern buffer."""
    if a.dtype == np.uint16:
        return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return a


def nan_buf(rows: int, dim: int, dtype: str = "f32", guard: int = GUARD) -> np.ndarray:
    """(rows + guard, dim) NaN-filled (dim = 0: a vector of rows + 16 * guard); int32 buffers hold INT_FILL."""
    shape = (rows + guard, dim) if dim else (rows + 16 * guard,)
    if dtype == "i32":
        return np.full(shape, INT_FILL, np.int32)
    if dtype == "bf16":
        return np.full(shape, 0x7FC0, np.uint16)
    return np.full(shape, np.nan, np.float32)


def bits(a: np.ndarray) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@dataclass
class Exact:
    """The first len(want) rows of the buffer hold ``want`` bit for bit (rows: only these are written); the rest keeps init."""
    want: np.ndarray
    rows: np.ndarray = None


@dataclass
class Bounded:
    """|buffer[:len(ref)] - ref| <= bound per element; the rest keeps init.  sim = the plain fp32 numpy evaluation.
    dtype bf16: the buffer holds bf16 patterns of such values."""
    ref: np.ndarray
    bound: np.ndarray
    sim: np.ndarray = None


@dataclass
class Scratch:
    """Work space of n elements the kernel may fill as it likes; everything behind it keeps init."""
    n: int


def want_full(e, init: np.ndarray) -> np.ndarray:
    full = init.copy()
    if isinstance(e, Exact):
        w = np.asarray(e.want).reshape((-1,) + init.shape[1:])
        assert w.dtype == init.dtype, (w.dtype, init.dtype)
        if e.rows is None:
            full[:len(w)] = w
        else:
            full[:len(w)][e.rows] = w[e.rows]
    return full


def judge(expected: dict, got: dict, init: dict):
    """-> ({output: worst error / bound}, [failures]).  An exact output scores 0 when every bit of the buffer is right."""
    ratios, fails = {}, []
    for name, e in expected.items():
        g, i = np.asarray(got[name]), init[name]
        if g.shape != i.shape or g.dtype != i.dtype:
            fails.append(f"{name}: buffer {g.dtype}{g.shape}, expected {i.dtype}{i.shape}")
            ratios[name] = math.inf
            continue
        if isinstance(e, Exact):
            w = want_full(e, i)
            bad = bits(g) != bits(w)
            ratios[name] = 0.0
            if bad.any():
                at = tuple(int(v) for v in np.argwhere(bad)[0])
                where = "guard / untouched" if at[0] >= len(np.asarray(e.want).reshape((-1,) + i.shape[1:])) else "output"
                fails.append(f"{name}: {int(bad.sum())} of {bad.size} elements differ, first at {at} ({where}): "
                             f"got {bits(g)[at]:#x}, expected {bits(w)[at]:#x}")
                ratios[name] = math.inf
            continue
        n = e.n if isinstance(e, Scratch) else len(np.asarray(e.ref).reshape((-1,) + i.shape[1:]))
        if (bits(g[n:]) != bits(i[n:])).any():
            fails.append(f"{name}: elements behind the {n} specified ones were written")
            ratios[name] = math.inf
            continue
        if isinstance(e, Scratch):
            continue
        ref = np.asarray(e.ref, np.float64).reshape((-1,) + i.shape[1:])
        bound = np.broadcast_to(np.asarray(e.bound, np.float64), ref.shape)
        val = from_dt(g[:n]).astype(np.float64)
        err = np.abs(val - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / bound)
        r = np.where(np.isfinite(val), r, math.inf)
        ratios[name] = float(np.max(r)) if r.size else 0.0
        if not ratios[name] <= 1.0:
            at = tuple(int(v) for v in np.argwhere(~(r <= 1.0))[0])
            fails.append(f"{name}: error / bound {ratios[name]:.3g} at {at}: got {val[at]!r}, reference {ref[at]!r}, bound {bound[at]:.3g}")
    return ratios, fails


def simulate(expected: dict, init: dict) -> dict:
    """What a correct kernel leaves behind: exact outputs as specified, bounded ones from the plain fp32 numpy evaluation."""
    out = {}
    for name, e in expected.items():
        full = init[name].copy()
        if isinstance(e, Exact):
            full = want_full(e, init[name])
        elif isinstance(e, Bounded):
            s = np.asarray(e.sim).reshape((-1,) + full.shape[1:])
            full[:len(s)] = s if s.dtype == full.dtype else to_dt(s, "bf16")
        out[name] = full
    return out


def colsum(x: np.ndarray, c: int, exact: bool, dtype: str = "f32"):
    """Exact | Bounded for the column sums of the rows x (n, D): float64 reference, bound c u sum|x|, fp32 sim row by row."""
    x = np.asarray(x, np.float32).reshape(-1, x.shape[-1])
    ref = x.astype(np.float64).sum(0)
    sim = np.zeros(x.shape[1], np.float32)
    for blk in np.array_split(x, max(1, len(x) // 4096)):   # fp32, sequential over chunks of pairwise sums
        sim = sim + blk.sum(0, dtype=np.float32)
    if exact:
        assert float(np.abs(x).astype(np.float64).sum(0).max(initial=0.0)) < 2.0 ** 24 and np.all(x == np.rint(x)) and np.all(np.abs(x) <= 8)
        return Exact(to_dt(ref.astype(np.float32), dtype))
    bound = c * U * np.abs(x).astype(np.float64).sum(0)
    if dtype == "bf16":
        bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)   # bf16 keeps 8 significant bits
    return Bounded(ref, bound, to_dt(sim, dtype))


def split_chain(rows: int, D: int) -> int:
    """c of the module docstring for the two-stage column sums over `rows` candidate rows."""
    R = rpi(D)
    G = min(cdiv(rows, R), SPLIT_BLOCKS)
    return cdiv(rows, G * R) + (R - 1) + cdiv(G, 32) + 32


# ------------------------------------------------------------------------------------------------ MAE row kernels
@dataclass(frozen=True)
class RowCase:
    id: str
    B: int
    L: int
    k: int
    D: int
    dtype: str      # activation type of xdec / dtok / d_xdec
    keep: str       # cls | all | sorted | unsorted

    @property
    def vis_rows(self):
        return self.B * self.k

    @property
    def dec_rows(self):
        return self.B * self.L


def row_cases():
    """D: 8 (128 rows per pass), 144 (RPI 7, 4 idle threads), 192 (RPI 5), 768 and 1024 (RPI 1, with and without idle threads).
    Rows: 1; k = 1; exactly G RPI with nothing masked; one more; 2.55 strides of 512 RPI (the U = 4 tail); more than
    4 * 512 * RPI (second trip of the split kernels) with a quarter kept and with everything kept; at D = 192 the second trips of
    decoder_assemble's and assemble_visible's 4096-block grids."""
    out = []
    for D in DIMS:
        R, L = rpi(D), 145
        tail_B, trip_B = cdiv(int(2.55 * SPLIT_BLOCKS * R), L), 4 * SPLIT_BLOCKS * R // L + 1
        table = [("one", 1, 1, 1, "cls", ("f32",)), ("clsonly", 3, 2 * R + 1, 1, "cls", ("f32",)),
                 ("exactGR", 1, 3 * R, 3 * R, "all", ("f32",)), ("GRplus1", 1, 3 * R + 1, max(1, (3 * R + 1) // 4), "sorted", ("f32", "bf16")),
                 ("tail", tail_B, L, 37, "unsorted", ("f32", "bf16")), ("tailall", tail_B, L, L, "all", ("f32",)),
                 ("trip", trip_B, L, 37, "sorted", ("f32", "bf16")), ("tripall", trip_B, L, L, "all", ("f32",))]
        if D == 192:
            table += [("grid2dec", 566, L, 37, "unsorted", ("f32",)), ("grid2vis", 152, L, L, "all", ("f32",))]
        for name, B, Lc, k, keep, dts in table:
            out += [RowCase(f"D{D}-{name}-{dt}", B, Lc, k, D, dt, keep) for dt in dts]
    return out


def _seed(cid: str) -> int:
    return int.from_bytes(cid.encode(), "little") % (2 ** 32)


def _values(rng, exact):
    if exact:
        return lambda *s: rng.integers(-8, 9, size=s).astype(np.float32)
    return lambda *s: rng.standard_normal(s, dtype=np.float32)


def make_keep(B, L, k, kind, rng):
    """(keep (B, k), mask (B, L - k)) int32: distinct ids per image."""
    keep = np.zeros((B, k), np.int32)
    mask = np.zeros((B, L - k), np.int32)
    for b in range(B):
        perm = rng.permutation(np.arange(1, L, dtype=np.int32))
        if kind == "unsorted" and k < L and b % 2:      # no class token at all in the odd images
            row = perm[:k]
        else:
            row = np.concatenate([[0], perm[:k - 1]]).astype(np.int32)
            if kind == "sorted":
                row = np.sort(row)
            elif kind == "unsorted":
                row = rng.permutation(row)                  # the class token anywhere
        keep[b] = row
        mask[b] = rng.permutation(np.setdiff1d(np.arange(L, dtype=np.int32), row))
    return keep, mask


def gen_rows(c: RowCase, exact: bool = False) -> dict:
    rng = np.random.default_rng(_seed(c.id) + exact)
    v = _values(rng, exact)
    keep, mask = make_keep(c.B, c.L, c.k, c.keep, rng)
    return dict(keep=keep, mask=mask, inv=ref_build_inverse(keep, c.L), x=v(c.vis_rows, c.D), cls=v(c.D), pos=v(c.L, c.D),
                dx_vis=v(c.vis_rows, c.D), xdec=to_dt(v(c.vis_rows, c.D), c.dtype), mask_token=v(c.D), dpos=v(c.L, c.D),
                dx_dec=v(c.dec_rows, c.D))


def ref_build_inverse(keep, L):
    B, k = keep.shape
    inv = np.full((B, L), -1, np.int32)
    for b in range(B):
        ok = (keep[b] >= 0) & (keep[b] < L)
        inv[b, keep[b][ok]] = np.arange(k, dtype=np.int32)[ok]
    return inv


def ref_build_row_map(idx, L):
    B = idx.shape[0]
    return (np.arange(B, dtype=np.int64)[:, None] * L + np.clip(idx, 0, L - 1)).astype(np.int32).reshape(-1)


def ref_assemble_visible(x, tok, cls, pos):
    t = tok.reshape(-1)
    base = np.where((t == 0)[:, None], cls[None, :], x)
    return base + pos[t]                                   # float32 + float32: one rounding


def ref_decoder_input(xdec32, inv, mask_token, pos):
    """(B * L, D) fp32: the visible rows scattered back, the mask token elsewhere, plus the position row."""
    B, L = inv.shape
    k = xdec32.shape[0] // B
    src = np.arange(B, dtype=np.int64)[:, None] * k + np.maximum(inv, 0)
    base = np.where((inv >= 0).reshape(-1, 1), xdec32[src.reshape(-1)], mask_token[None, :])
    return base + np.tile(pos, (B, 1))


def row_inits(c: RowCase, d: dict) -> dict:
    x = nan_buf(c.vis_rows, c.D)
    x[:c.vis_rows] = d["x"]
    return {"build_inverse.inv": nan_buf(c.dec_rows, 0, "i32"), "build_row_map.rows": nan_buf(c.B * (c.L - c.k), 0, "i32"),
            "assemble_visible.x": x, "visible_grad_split.dtok": nan_buf(c.vis_rows, c.D, c.dtype),
            "visible_grad_split.dcls": nan_buf(c.D, 0), "visible_grad_split.partial": nan_buf(PARTIAL_BLOCKS * c.D, 0),
            "decoder_assemble.out": nan_buf(c.dec_rows, c.D), "decoder_assemble_bwd.d_xdec": nan_buf(c.vis_rows, c.D, c.dtype),
            "decoder_assemble_bwd.d_mask_token": nan_buf(c.D, 0), "decoder_assemble_bwd.partial": nan_buf(PARTIAL_BLOCKS * c.D, 0)}


def expect_rows(c: RowCase, d: dict, exact: bool = False) -> dict:
    keep, inv = d["keep"], d["inv"]
    is_cls = keep.reshape(-1) == 0
    dtok = d["dx_vis"].copy()
    dtok[is_cls] = 0.0
    masked = (inv < 0).reshape(-1)
    d_xdec = np.zeros((c.vis_rows, c.D), np.float32)
    dst = (np.arange(c.B, dtype=np.int64)[:, None] * c.k + inv).reshape(-1)
    d_xdec[dst[~masked]] = d["dx_dec"][~masked]
    e = {"build_inverse.inv": Exact(inv.reshape(-1)),
         "assemble_visible.x": Exact(ref_assemble_visible(d["x"], keep, d["cls"], d["pos"])),
         "visible_grad_split.dtok": Exact(to_dt(dtok, c.dtype)),
         "visible_grad_split.dcls": colsum(d["dx_vis"][is_cls], split_chain(c.vis_rows, c.D), exact),
         "visible_grad_split.partial": Scratch(PARTIAL_BLOCKS * c.D),
         "decoder_assemble.out": Exact(ref_decoder_input(from_dt(d["xdec"]), inv, d["mask_token"], d["dpos"])),
         "decoder_assemble_bwd.d_xdec": Exact(to_dt(d_xdec, c.dtype)),
         "decoder_assemble_bwd.d_mask_token": colsum(d["dx_dec"][masked], split_chain(c.dec_rows, c.D), exact),
         "decoder_assemble_bwd.partial": Scratch(PARTIAL_BLOCKS * c.D)}
    if c.k < c.L:
        e["build_row_map.rows"] = Exact(ref_build_row_map(d["mask"], c.L))
    if c.k == c.L:    # nothing masked: exact zeros whatever the inputs
        e["decoder_assemble_bwd.d_mask_token"] = Exact(np.zeros(c.D, np.float32))
    return e


# ------------------------------------------------------------------------------------------------ zero_unpredicted_rows
@dataclass(frozen=True)
class ZeroCase:
    id: str
    D: int
    B: int
    T: int          # rows per sequence
    m: int          # predicted rows per sequence (the last m); with an inv map: T - m rows are kept, at random places
    use_inv: bool
    dtype: str


def zero_cases():
    """D 192 (48 of 64 lanes), 256 (64 lanes exactly), 264 (128 lanes, partial second pass), 1024 (two full passes); both modes;
    m in {0, 1, T}; more than 8192 * rpb rows (rpb 4 at D 192, 2 at D 264)."""
    out = []
    for D in (192, 256, 264, 1024):
        for dt in ("f32", "bf16"):
            out.append(ZeroCase(f"D{D}-inv-{dt}", D, 3, 50, 37, True, dt))
        for m in (0, 1, 50):
            out.append(ZeroCase(f"D{D}-tail-m{m}", D, 3, 50, m, False, "f32" if m else "bf16"))
    out += [ZeroCase("D192-tail-trip", 192, 328, 100, 20, False, "f32"), ZeroCase("D264-inv-trip", 264, 114, 145, 108, True, "bf16"),
            ZeroCase("D264-tail-trip", 264, 165, 100, 20, False, "f32")]
    return out


def gen_zero(c: ZeroCase) -> dict:
    rng = np.random.default_rng(_seed(c.id))
    inv = None
    if c.use_inv:
        keep, _ = make_keep(c.B, c.T, c.T - c.m, "unsorted", rng)
        inv = ref_build_inverse(keep, c.T)
    rows = c.B * c.T
    return dict(inv=inv, dres=rng.standard_normal((rows, c.D), dtype=np.float32), dres_c=to_dt(rng.standard_normal((rows, c.D), dtype=np.float32), c.dtype))


def zero_inits(c: ZeroCase, d: dict) -> dict:
    rows = c.B * c.T
    a, b = nan_buf(rows, c.D), nan_buf(rows, c.D, c.dtype)
    a[:rows], b[:rows] = d["dres"], d["dres_c"]
    return {"zero_unpredicted_rows.dres": a, "zero_unpredicted_rows.dres_c": b}


def expect_zero(c: ZeroCase, d: dict) -> dict:
    rows = c.B * c.T
    clear = (d["inv"].reshape(-1) >= 0) if c.use_inv else (np.arange(rows) % c.T < c.T - c.m)
    a, b = d["dres"].copy(), d["dres_c"].copy()
    a[clear], b[clear] = 0, 0
    return {"zero_unpredicted_rows.dres": Exact(a), "zero_unpredicted_rows.dres_c": Exact(b)}


# ------------------------------------------------------------------------------------------------ I-JEPA predictor rows
@dataclass(frozen=True)
class JepaCase:
    id: str
    B: int
    k: int          # context tokens
    nblk: int
    m: int          # tokens per target block
    L: int
    D: int
    dtype: str

    @property
    def rows(self):
        return self.B * self.nblk * (self.k + self.m)


JEPA_BIG_B = {8: 1320, 144: 72, 192: 52, 768: 11, 1024: 11}   # second trips: assemble rows > 4096 rpb, context and mask rows > 512 RPI


def jepa_cases():
    out = []
    for D in DIMS:
        R = rpi(D)
        table = [("one", 1, 1, 1, 1, 5, ("f32",)), ("exactGR", 1, 3 * R - 1, 1, 1, 3 * R + 4, ("f32",)), ("GRplus1", 1, 3 * R, 1, 1, 3 * R + 4, ("f32", "bf16")),
                 ("blocks", 3, 7, 4, 20, 50, ("f32", "bf16")), ("m1", 2, 9, 4, 1, 50, ("f32",)), ("trip", JEPA_BIG_B[D], 80, 4, 20, 197, ("f32",))]
        for name, B, k, nblk, m, L, dts in table:
            out += [JepaCase(f"D{D}-{name}-{dt}", B, k, nblk, m, L, D, dt) for dt in dts]
    return out


def gen_jepa(c: JepaCase, exact: bool = False) -> dict:
    rng = np.random.default_rng(_seed(c.id) + exact)
    v = _values(rng, exact)
    return dict(ctx=rng.integers(1, c.L, size=(c.B, c.k)).astype(np.int32), tgt=rng.integers(1, c.L, size=(c.B, c.nblk, c.m)).astype(np.int32),
                xdec=to_dt(v(c.B * c.k, c.D), c.dtype), mask_token=v(c.D), pos=v(c.L, c.D), dx=v(c.rows, c.D))


def ref_predictor_input(xdec32, ctx, tgt, mask_token, pos):
    B, k = ctx.shape
    _, nblk, m = tgt.shape
    D = xdec32.shape[1]
    out = np.empty((B, nblk, k + m, D), np.float32)
    out[:, :, :k] = (xdec32.reshape(B, k, D) + pos[ctx])[:, None]
    out[:, :, k:] = mask_token[None, None, None, :] + pos[tgt]
    return out.reshape(-1, D)


def jepa_inits(c: JepaCase, d: dict) -> dict:
    return {"predictor_assemble.out": nan_buf(c.rows, c.D), "predictor_assemble_bwd.d_xdec": nan_buf(c.B * c.k, c.D, c.dtype),
            "predictor_assemble_bwd.d_mask_token": nan_buf(c.D, 0), "predictor_assemble_bwd.partial": nan_buf(PARTIAL_BLOCKS * c.D, 0),
            "build_tail_row_map.rows": nan_buf(c.B * c.nblk * c.m, 0, "i32"), "rows_from_tokens.rows": nan_buf(c.B * c.nblk * c.m, 0, "i32")}


def ref_tail_row_map(seqs, T, m):
    return (np.arange(seqs, dtype=np.int64)[:, None] * T + (T - m) + np.arange(m)).astype(np.int32).reshape(-1)


def ref_rows_from_tokens(tok, per_image, N):
    t = tok.reshape(-1).astype(np.int64)
    return ((np.arange(t.size) // per_image) * N + np.clip(t - 1, 0, N - 1)).astype(np.int32)


def expect_jepa(c: JepaCase, d: dict, exact: bool = False) -> dict:
    dx = d["dx"].reshape(c.B, c.nblk, c.k + c.m, c.D)
    ctx_rows = dx[:, :, :c.k]                                       # (B, nblk, k, D)
    ref = ctx_rows.astype(np.float64).sum(1).reshape(-1, c.D)
    sim = np.zeros((c.B, c.k, c.D), np.float32)
    for blk in range(c.nblk):
        sim = sim + ctx_rows[:, blk]
    if exact:
        d_xdec = Exact(to_dt(ref.astype(np.float32), c.dtype))
    else:
        bound = c.nblk * U * np.abs(ctx_rows).astype(np.float64).sum(1).reshape(-1, c.D)
        if c.dtype == "bf16":
            bound = bound + 2.0 ** -8 * (np.abs(ref) + bound)   # bf16 keeps 8 significant bits
        d_xdec = Bounded(ref, bound, to_dt(sim.reshape(-1, c.D), c.dtype))
    R, n_mask = rpi(c.D), c.B * c.nblk * c.m
    G = min(cdiv(max(c.B * c.k, n_mask), R), SPLIT_BLOCKS)
    chain = cdiv(n_mask, G * R) + (R - 1) + cdiv(G, 32) + 32
    return {"predictor_assemble.out": Exact(ref_predictor_input(from_dt(d["xdec"]), d["ctx"], d["tgt"], d["mask_token"], d["pos"])),
            "predictor_assemble_bwd.d_xdec": d_xdec,
            "predictor_assemble_bwd.d_mask_token": colsum(dx[:, :, c.k:].reshape(-1, c.D), chain, exact),
            "predictor_assemble_bwd.partial": Scratch(PARTIAL_BLOCKS * c.D),
            "build_tail_row_map.rows": Exact(ref_tail_row_map(c.B * c.nblk, c.k + c.m, c.m)),
            "rows_from_tokens.rows": Exact(ref_rows_from_tokens(d["tgt"], c.nblk * c.m, c.L - 1))}


# the three grid-stride index kernels past their 2048-block grids (524288 elements): (kernel, arguments)
INDEX_TRIPS = (("build_row_map", dict(B=4855, n_per=108, L=145)), ("build_tail_row_map", dict(seqs=26215, T=100, m=20)),
               ("rows_from_tokens", dict(B=6555, per_image=80, N=196)))


# ------------------------------------------------------------------------------------------------ pixels
def norm_u8(u) -> np.ndarray:
    """ToTensor + Normalize(.5, .5) of a uint8 pixel in fp32: (fl(u / 255) - 0.5) / 0.5."""
    return (np.asarray(u).astype(np.float32) / f32(255.0) - f32(0.5)) / f32(0.5)


def patches_of(images32, p, order):
    """(B, g*g, P) fp32 view of the patches of (B, C, S, S) images: order 'cpp' = (c, py, px) (the conv weight's), 'ppc' = (py, px, c)."""
    B, C, S, _ = images32.shape
    g = S // p
    x = images32.reshape(B, C, g, p, g, p)
    x = x.transpose(0, 2, 4, 1, 3, 5) if order == "cpp" else x.transpose(0, 2, 4, 3, 5, 1)
    return np.ascontiguousarray(x).reshape(B, g * g, C * p * p)


def u8_supported(C, img, p, n_tok) -> bool:
    return p % 4 == 0 and img // p <= 64 and C * p * img <= 96 * 1024 and n_tok <= 8192


def band_f32_eligible(C, img, p, m) -> bool:
    """Geometries launch_mse_from_images serves with the float band walk (16-byte aligned buffers assumed)."""
    return p % 4 == 0 and img // p <= 64 and C * p * img * 4 <= 96 * 1024 and m <= 8192 and (C * p * p) % 4 == 0


U8_GATHER_MESSAGE = "uint8 images need patch_size % 4 == 0 and at most 64 patches per side"
U8_LOSS_MESSAGE = "uint8 images: unsupported geometry"


@dataclass(frozen=True)
class PixCase:
    id: str
    C: int
    img: int
    p: int
    B: int
    n: int          # tokens per image (visible ones for the gather, masked ones for the loss)
    kind: str       # random | oneband | emptyband | all | oor (loss only: ids 0 and g*g + 1)
    lite: bool = False

    @property
    def g(self):
        return self.img // self.p

    @property
    def P(self):
        return self.C * self.p * self.p


GEOS = ((3, 32, 8), (3, 96, 8), (1, 16, 4), (1, 28, 7), (3, 42, 14))


def gather_cases():
    out = []
    for C, img, p in GEOS:
        g = img // p
        out += [PixCase(f"c{C}i{img}p{p}-{kind}", C, img, p, 3, n, kind) for kind, n in
                (("random", g * g // 4 + 1), ("oneband", 2 * g + 1), ("emptyband", g + 2), ("all", g * g + 1))]
    out += [PixCase("c1i16p4-B1025", 1, 16, 4, 1025, 5, "random", True),        # B g = 4100 > the uint8 gather's 4096 blocks
            PixCase("c3i32p8-B1300", 3, 32, 8, 1300, 17, "all", True),          # 1.06 M vector units > the float gather's 4096 x 256
            PixCase("c3i1024p16-all", 3, 1024, 16, 1, 4097, "all", True),       # band + list = 65540 bytes of LDS
            PixCase("c1i260p4-g65", 1, 260, 4, 1, 6, "random", True)]           # 65 patches per side: the uint8 walk declines
    return out


def loss_cases():
    out = []
    for C, img, p in GEOS:
        g = img // p
        out += [PixCase(f"c{C}i{img}p{p}-{kind}", C, img, p, 3, n, kind) for kind, n in
                (("random", g * g - g * g // 4), ("oneband", 2 * g + 1), ("emptyband", g + 2), ("oor", g + 3))]
    out += [PixCase("c3i32p8-B257", 3, 32, 8, 257, 12, "random", True),         # B g = 1028 > 1024 blocks
            PixCase("c1i28p7-B300", 1, 28, 7, 300, 12, "oor", True),            # the gather past one block, out-of-range ids
            PixCase("c3i1024p16-all", 3, 1024, 16, 1, 4096, "all", True),       # band + two lists = 81920 bytes of LDS
            PixCase("c1i260p4-g65", 1, 260, 4, 1, 6, "oor", True)]              # 65 patches per side: both band walks decline
    return out


def make_tokens(c: PixCase, rng, with_cls: bool) -> np.ndarray:
    """(B, n) int32 token ids (0 = class token, t = patch t - 1); ids outside [0, g*g] only for kind oor."""
    g, N = c.g, c.g * c.g
    tok = np.zeros((c.B, c.n), np.int32)
    for b in range(c.B):
        if c.kind == "all":
            row = rng.permutation(np.arange(0 if with_cls else 1, N + 1))[:c.n]
        elif c.kind == "oneband":       # every token in patch row g - 1 (ids repeat)
            row = (g - 1) * g + rng.integers(0, g, size=c.n) + 1
        elif c.kind == "emptyband":     # nothing in patch row 1
            pool = np.array([t for t in range(1, N + 1) if (t - 1) // g != 1])
            row = rng.choice(pool, size=c.n, replace=c.n > len(pool))
        else:
            row = rng.integers(1, N + 1, size=c.n)
        row = np.asarray(row, np.int32)
        if c.kind == "oor":
            row[0], row[1], row[-1] = 0, N + 1, N + 1
        elif with_cls and c.kind != "oneband" and c.kind != "all":
            row[rng.integers(0, c.n)] = 0
        tok[b] = row
    return tok


def gen_pixels(c: PixCase, with_cls: bool) -> dict:
    """u8 images (B + 1: a spare image of 255 behind the batch), their normalised fp32 form (spare = NaN), tokens, pred."""
    rng = np.random.default_rng(_seed(c.id) + with_cls)
    u8 = rng.integers(0, 256, size=(c.B + 1, c.C, c.img, c.img), dtype=np.uint8)
    u8[c.B] = 255
    f = norm_u8(u8)
    f[c.B] = np.nan
    return dict(u8=u8, f32=f, tok=make_tokens(c, rng, with_cls), pred=rng.standard_normal((c.B * c.n, c.P), dtype=np.float32))


def expect_gather(c: PixCase, d: dict, out_dtype: str) -> dict:
    """Both image dtypes give the same rows: the fp32 images are norm_u8 of the uint8 ones."""
    pat = patches_of(d["f32"][:c.B], c.p, "cpp")
    tok = d["tok"]
    rows = pat[np.arange(c.B)[:, None], np.maximum(tok - 1, 0)]
    rows[tok <= 0] = 0.0
    return {"gather_patches.out": Exact(to_dt(rows.reshape(-1, c.P), out_dtype))}


def gather_inits(c: PixCase, out_dtype: str) -> dict:
    return {"gather_patches.out": nan_buf(c.B * c.n, c.P, out_dtype)}


def mse_gs(grad_scale, n: int) -> np.float32:
    return f32(grad_scale) * f32(2.0) / f32(n)


def loss_bound(chain: int, ref: float) -> float:
    return (chain + 3) * U * ref


def mse_chain(c: PixCase, tok, variant: str) -> int:
    """c of the module docstring; variant 'gather' or 'band' (uint8 and float band walks share the loop)."""
    g = c.g
    if variant == "gather":
        units = c.B * c.n * c.p * c.p
        grid = min(cdiv(units, 256), RED_BLOCKS)
        A = cdiv(units, grid * 256) * c.C
    else:
        grid = min(c.B * g, RED_BLOCKS)
        band = np.clip(tok - 1, 0, g * g - 1) // g                       # (B, n) patch row of every token
        per_band = np.stack([(band == ph).sum(1) for ph in range(g)], 1).reshape(-1)   # tokens of band bb = b g + ph
        adds = -(-per_band * (c.p * (c.p // 4)) // 256) * 4 * c.C
        A = max(int(adds[blk::grid].sum()) for blk in range(grid))
    return A + 6 + 3 + cdiv(grid, 256) + 6 + 3


def mse_variant(c: PixCase, image_dtype: str, path: int) -> str:
    if image_dtype == "u8":
        return "band"
    return "band" if path == 0 and band_f32_eligible(c.C, c.img, c.p, c.n) else "gather"


def loss_inits(c: PixCase, dp: str) -> dict:
    out = {"mse.loss": nan_buf(1, 0), "mse.scratch": nan_buf(SCRATCH_FLOATS, 0)}
    if dp:
        out["mse.d_pred"] = nan_buf(c.B * c.n, c.P, dp)
    return out


def target_rows(c: PixCase, d: dict) -> np.ndarray:
    """(B * n, P) fp32: patch clamp(id - 1, 0, g*g - 1) of every token in (py, px, c) order.  Both image dtypes give the same rows."""
    pat = patches_of(d["f32"][:c.B], c.p, "ppc")
    idx = np.clip(d["tok"] - 1, 0, c.g * c.g - 1)
    return pat[np.arange(c.B)[:, None], idx].reshape(-1, c.P)


def patchify_inits(c: PixCase) -> dict:
    return {"patchify_gather.target": nan_buf(c.B * c.n, c.P)}


def expect_patchify(c: PixCase, d: dict) -> dict:
    """A copy: no arithmetic on float images, norm_u8 alone on uint8 ones."""
    return {"patchify_gather.target": Exact(target_rows(c, d))}


def expect_mse(c: PixCase, d: dict, variant: str, grad_scale, dp: str) -> dict:
    """dp: '' (d_pred NULL) | 'f32' | 'bf16'.  The target is patch clamp(id - 1, 0, g*g - 1) in (py, px, c) order."""
    t = target_rows(c, d)
    n = t.size
    diff = d["pred"] - t
    ref = float(((d["pred"].astype(np.float64) - t.astype(np.float64)) ** 2).sum() / n)
    sim = f32((diff * diff).sum(dtype=np.float32) * (f32(1.0) / f32(n)))
    e = {"mse.loss": Bounded(np.array([ref]), np.array([loss_bound(mse_chain(c, d["tok"], variant), ref)]), np.array([sim], np.float32)),
         "mse.scratch": Scratch(SCRATCH_FLOATS)}
    if dp:
        e["mse.d_pred"] = Exact(to_dt(diff * mse_gs(grad_scale, n), dp))
    return e


# ------------------------------------------------------------------------------------------------ smooth L1
ONE_M, ONE_P = float(1 - 2.0 ** -24), float(1 + 2.0 ** -23)
SL1_SPECIALS = np.array([0.0, 1.0, -1.0, ONE_M, -ONE_M, ONE_P, -ONE_P, 1e6, -3.5e4, -0.0, 0.25, -0.75], np.float32)


@dataclass(frozen=True)
class Sl1Case:
    id: str
    n: int


def sl1_cases():
    """n = 4; one block; exactly 1024 blocks; a second trip (with a part-filled last pass)."""
    return [Sl1Case("n4", 4), Sl1Case("n12", 12), Sl1Case("oneblock", 1000), Sl1Case("blocks1024", 1024 * 1024), Sl1Case("trip2", 1024 * 1024 + 2052)]


def gen_sl1(c: Sl1Case) -> dict:
    rng = np.random.default_rng(_seed(c.id))
    pred = (rng.standard_normal(c.n, dtype=np.float32) * f32(1.5)).astype(np.float32)
    target = rng.standard_normal(c.n, dtype=np.float32)
    s = SL1_SPECIALS[:min(c.n, len(SL1_SPECIALS))] if c.n > 4 else np.array([1.0, -ONE_M, ONE_P, 0.0], np.float32)
    pred[:len(s)], target[:len(s)] = s, 0.0             # the differences are these values exactly
    return dict(pred=pred, target=target)


def sl1_chain(n: int) -> int:
    n4 = n // 4
    grid = min(cdiv(n4, 256), RED_BLOCKS)
    return cdiv(n4, grid * 256) * 4 + 6 + 3 + cdiv(grid, 256) + 6 + 3


def sl1_inits(c: Sl1Case, dp: str) -> dict:
    out = {"smooth_l1.loss": nan_buf(1, 0), "smooth_l1.scratch": nan_buf(SCRATCH_FLOATS, 0)}
    if dp:
        out["smooth_l1.d_pred"] = nan_buf(c.n, 0, dp)
    return out


def expect_sl1(c: Sl1Case, d: dict, grad_scale, dp: str) -> dict:
    diff = d["pred"] - d["target"]
    d64 = d["pred"].astype(np.float64) - d["target"].astype(np.float64)
    a = np.abs(d64)
    ref = float(np.where(a < 1.0, 0.5 * d64 * d64, a - 0.5).sum() / c.n)
    a32 = np.abs(diff)
    sim = f32(np.where(a32 < 1, f32(0.5) * diff * diff, a32 - f32(0.5)).sum(dtype=np.float32) * (f32(1.0) / f32(c.n)))
    e = {"smooth_l1.loss": Bounded(np.array([ref]), np.array([loss_bound(sl1_chain(c.n), ref)]), np.array([sim], np.float32)),
         "smooth_l1.scratch": Scratch(SCRATCH_FLOATS)}
    if dp:
        gs = f32(grad_scale) / f32(c.n)
        e["smooth_l1.d_pred"] = Exact(to_dt(np.clip(diff, f32(-1), f32(1)) * gs, dp))
    return e
