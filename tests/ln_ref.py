"""float64 restatement of LayerNorm forward / backward (k_layernorm.hip) and of the second stage of its column reductions
(sum_partials_kernel in k_patch.hip) for the tests, the launch geometry of both, per-element error bounds of the fp32 kernels,
and the case table the host and the GPU tests share.

numpy on the CPU, float64 throughout.  bf16 tensors are held as fp32 arrays whose values are bf16 numbers.

Indexing, as the kernels document it.  ``rows`` compact rows; with a row map, compact row r belongs to row src = row_map[r] of the
full matrix, without one src = r.
  forward    reads x[src] (+ branch[src]); writes x_out[src] = fl32(x[src] + branch[src]), y[r], mean[r], rstd[r]
  backward   reads dy[r], mean[r], rstd[r], x[src]; writes dx[src] (+= with accumulate), dx_copy[src]; dgamma / dbeta are column
             sums over the compact rows
The LayerNorm of the fused add is taken of the fp32 value written to x_out, so the reference rounds the sum to fp32 first.

Geometry.  A row of d4 = dim / 4 float4 is held by lpr = ln_lanes_per_row(d4) consecutive lanes, NV = ceil(d4 / lpr) vectors per
lane (vector i of lane li is float4 column li + lpr i), R = 64 / lpr rows per wave and trip, 4 waves per block.  Wave w of block b
takes rows (4 b + w) R .. + R - 1 and strides by grid 4 R rows; forward grid = min(ceil(rows / 4R), 8192), backward grid G =
min(ceil(rows / 4R), LN_BWD_MAX_BLOCKS).  A lane group keeps its dgamma / dbeta column partials over its trips, the block writes
them to LDS as red[4 R groups][2][dim] and adds the 4 R groups in order into partial[b][2 dim]; sum_partials then gives 32 columns
to a block, row lane rl adds partial rows rl, rl + 32, .. in order and the 32 row lanes are added in order.

Bounds.  u = 2^-24; every fp32 operation returns x (1 + d), |d| <= u; a value that went through k of them is off by at most k u
to first order and the factor SECOND = 1 + 2^-16 covers the second order (k <= 100 here).  Fused multiply-adds (-ffp-contract=fast)
only remove roundings from a chain.  All counts need normal numbers (or exact zeros).  L = log2(lpr).
  mean   ((v0 + v1) + v2) + v3 inside a float4 = 3, one `sum +=` per vector = NV, the shuffle butterfly = L, inv_d = fl(1 / dim)
         and the product = 2:                                   k = NV + L + 5,    |err| <= k u sum|v| / dim       =: bm
  var    the kernel sums (v - m)^2 about its own mean m = mean + e, which is dim (var + e^2) exactly.  fl(v - m) = 1, squared = 2,
         the square = 1, then 3 + NV + L + 2 as above:          k = NV + L + 8,    |err| <= k u (var + bm^2) + bm^2 =: bv
  rstd   fl(var + eps) = 1 on a positive sum, halved by the power -1/2, and the error of rsqrtf.  ROCm's table of device-function
         accuracy is not among the files of a ROCm installation, so RSQRT_ULP = 2 ulp = 4 u is allowed (not measured).  With
         t = bv / (var + eps) + u:                              rel = t (1 + t) / 2 + 4 u   (|(1 + t)^-1/2 - 1| <= t (1 + t) / 2)
  y      o = fl(fl(fl(fl(v - m) rstd) gamma) + beta), a = (v - mean) rstd gamma: the subtraction carries bm and 1, rstd rel + 1,
         gamma 1, the sum rounds |a| + |beta| once:
                                                                |err| <= |rstd gamma| bm + |a| (rel + 4 u) + u |beta|
         a bf16 output adds half a bf16 ulp of the result:      + 2^-8 (|y| + that bound)
  backward: mean and rstd are inputs there (exact).  xh = fl(fl(x - mu) rs) = 2, g = fl(dy gamma) = 1.
  s1     g 1 + 3 + NV + L + 2:                                  k = NV + L + 6,    |err| <= k u sum|g| / dim        =: b1
  s2     g xh: 1 + 2 + the product 1, then 3 + NV + L + 2:      k = NV + L + 9,    |err| <= k u sum|g xh| / dim     =: b2
  dx     fl(fl(fl(g - s1) - fl(xh s2)) rs): |g| is rounded as g, in both differences and in the product = 4; |s1| in both
         differences and the product = 3, plus b1; |xh s2| carries xh 2 and its own product 1, the second difference and the
         last product = 5, plus |xh| b2:
                                                                |err| <= |rs| (4 u |g| + 3 u |s1| + 5 u |xh s2| + b1 + |xh| b2)
         accumulate adds one rounding of the sum:               + u (|dx| + |residual|)
         dx_copy in bf16:                                       + 2^-8 (|value| + that bound)
  dgamma the term dy xh = 3 (none for dbeta), one `+=` per trip of the lane group = T, the serial LDS sum = 4 R, the strided
         second-stage sum = ceil(G / 32), its serial sum over row lanes = 32:
                                                                k = 3 + T + 4 R + ceil(G / 32) + 32,  |err| <= k u sum_r |dy xh|
  dbeta                                                         k = T + 4 R + ceil(G / 32) + 32,      |err| <= k u sum_r |dy|
Bounds are evaluated from the inputs and the float64 reference only.

Exact checks beside the bounds: x_out = fl32(x + branch) bit for bit; a constant row (const_value) has var = 0, so y = beta bit for
bit and rstd lies within RSQRT_ULP ulp of 1 / sqrt(eps) (the host cannot evaluate the device's rsqrtf, so "equal to fl(rsqrtf(eps))"
is stated as that window); the gen_exact data (small integers) gives dgamma and dbeta equal to the float64 sums at every dim
and, at power-of-two dims, dx, dx_copy and the forward mean as well.
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass

import numpy as np

from tests.optim_ref import bf16_rne

U = 2.0 ** -24
UB = 2.0 ** -8            # half a bf16 ulp, relative
SECOND = 1.0 + 2.0 ** -16
RSQRT_ULP = 2             # allowed error of rsqrtf in ulp (see the docstring)
EPS = 1e-6
FWD_MAX_BLOCKS, LN_BWD_MAX_BLOCKS = 256 * 32, 1024
SP_COLS, SP_LANES = 32, 32   # sum_partials: columns per block, row lanes
F = np.float32

# (lanes per row, NV, smallest dim, largest dim) of the eight instantiations ln_lanes_per_row can select
PAIRS = [(16, 1, 4, 64), (32, 1, 68, 128), (16, 3, 132, 192), (64, 1, 196, 256), (32, 3, 260, 384), (64, 2, 388, 512),
         (64, 3, 516, 768), (64, 4, 772, 1024)]
UNREACHABLE = [(16, 2), (16, 4), (32, 2), (32, 4)]   # never selected, not compiled: ties in the fill go to the wider group


def f32(x) -> float:
    return float(F(x))


def cdiv(a: int, b: int) -> int:
    return -(-a // b)


def _d(x) -> np.ndarray:
    return np.asarray(x, dtype=np.float64)


def to_bf16(x) -> np.ndarray:
    """fp32 array of the values rounded to bf16 (nearest even)."""
    x = np.ascontiguousarray(x, dtype=F)
    return (bf16_rne(x).astype(np.uint32) << np.uint32(16)).view(F).reshape(x.shape)


# ------------------------------------------------------------------------------------------------ geometry
def lanes_per_row(d4: int) -> int:
    """ln_lanes_per_row: the widest group that wastes no more lanes than a narrower one would."""
    best, best_fill = 64, d4 / (64.0 * cdiv(d4, 64))
    for lpr in (32, 16):
        if cdiv(d4, lpr) > 4:
            continue
        fill = d4 / (float(lpr) * cdiv(d4, lpr))
        if fill > best_fill + 1e-9:
            best_fill, best = fill, lpr
    return best


@dataclass(frozen=True)
class Geo:
    rows: int
    dim: int
    lpr: int
    nv: int
    rpw: int          # rows per wave and trip
    fwd_grid: int
    bwd_grid: int
    fwd_trips: int    # trips of the busiest wave
    bwd_trips: int
    lds_floats: int   # red[4 rpw][2][dim]
    sp_blocks: int    # blocks of the second stage (2 dim columns)
    sp_strided: int   # additions of one row lane of the second stage


def geometry(rows: int, dim: int) -> Geo:
    assert dim % 4 == 0 and 4 <= dim <= 1024 and rows > 0
    d4 = dim // 4
    lpr = lanes_per_row(d4)
    nv, rpw = cdiv(d4, lpr), 64 // lpr
    units = cdiv(rows, 4 * rpw)
    fg, bg = min(units, FWD_MAX_BLOCKS), min(units, LN_BWD_MAX_BLOCKS)
    return Geo(rows, dim, lpr, nv, rpw, fg, bg, cdiv(rows, fg * 4 * rpw), cdiv(rows, bg * 4 * rpw), 8 * rpw * dim,
               cdiv(2 * dim, SP_COLS), cdiv(bg, SP_LANES))


def lds_index(geo: Geo, wave: int, sub: int, which: int, col: int) -> int:
    """Float index in red[4 R lane groups][2][dim] of lane group (wave, sub)'s partial of column col; which = 0 dgamma, 1 dbeta."""
    return ((wave * geo.rpw + sub) * 2 + which) * geo.dim + col


def locate(geo: Geo, row: int, col: int, bwd: bool) -> str:
    """Where element (compact row, column) is computed: block, wave, lane group, lane, vector and trip."""
    grid = geo.bwd_grid if bwd else geo.fwd_grid
    unit, sub = divmod(row, geo.rpw)
    trip, gw = divmod(unit, grid * 4)
    c4 = col // 4
    return (f"row {row} col {col}: block {gw // 4} wave {gw % 4} lane group {sub} (of {geo.rpw}) lane {c4 % geo.lpr} vector {c4 // geo.lpr} "
            f"trip {trip} of {geo.bwd_trips if bwd else geo.fwd_trips}")


def locate_col(geo: Geo, col: int, second: bool) -> str:
    c = col + (geo.dim if second else 0)
    return f"col {col}: lane {(col // 4) % geo.lpr} vector {(col // 4) // geo.lpr}; second stage block {c // SP_COLS} column lane {(c % SP_COLS) // 4}"


# ------------------------------------------------------------------------------------------------ the operations, fp64
def _src(rows, row_map):
    return np.arange(rows) if row_map is None else np.asarray(row_map, dtype=np.int64)


def fwd_ref(x, gamma, beta, rows, row_map=None, branch=None, eps=EPS):
    """dict(x_out fp32 (compact rows; None without a branch), mean, var, rstd, y, d, asum = sum|v|) in float64."""
    src = _src(rows, row_map)
    xo = None
    v = _d(x[src])
    if branch is not None:
        xo = (v + _d(branch[src])).astype(F)
        v = _d(xo)
    dim = v.shape[1]
    mean = v.sum(1) / dim
    d = v - mean[:, None]
    var = (d * d).sum(1) / dim
    rstd = 1.0 / np.sqrt(var + f32(eps))
    y = d * rstd[:, None] * _d(gamma) + _d(beta)
    return dict(x_out=xo, mean=mean, var=var, rstd=rstd, y=y, d=d, asum=np.abs(v).sum(1))


def fwd_bounds(ref, geo: Geo, gamma, beta, bf16: bool, eps=EPS):
    """dict(mean, var, rstd, y) of bounds; the counts are in the module docstring."""
    L = int(math.log2(geo.lpr))
    bm = SECOND * (geo.nv + L + 5) * U * ref["asum"] / geo.dim
    bv = SECOND * ((geo.nv + L + 8) * U * (ref["var"] + bm * bm) + bm * bm)
    t = bv / (ref["var"] + f32(eps)) + U
    rel = SECOND * (0.5 * t * (1.0 + t) + RSQRT_ULP * 2.0 * U)
    a = ref["d"] * ref["rstd"][:, None] * _d(gamma)
    by = SECOND * (np.abs(ref["rstd"][:, None] * _d(gamma)) * bm[:, None] + np.abs(a) * (rel[:, None] + 4.0 * U) + U * np.abs(_d(beta)))
    if bf16:
        by = by + UB * (np.abs(ref["y"]) + by)
    return dict(mean=bm, var=bv, rstd=ref["rstd"] * rel, y=by)


def bwd_ref(dy, x, gamma, mean, rstd, rows, row_map=None, accumulate=0, res=None):
    """dict(dx (compact rows: the value written to dx[src], residual included), dgamma, dbeta and the terms the bounds need)."""
    src = _src(rows, row_map)
    dy, xs, mu, rs = _d(dy), _d(x[src]), _d(mean)[:, None], _d(rstd)[:, None]
    dim = xs.shape[1]
    xh = (xs - mu) * rs
    g = dy * _d(gamma)
    s1 = g.sum(1, keepdims=True) / dim
    s2 = (g * xh).sum(1, keepdims=True) / dim
    dxc = (g - s1 - xh * s2) * rs
    r = _d(res[src]) if accumulate else None
    return dict(dx=dxc + r if accumulate else dxc, dxc=dxc, res=r, dgamma=(dy * xh).sum(0), dbeta=dy.sum(0), xh=xh, g=g, s1=s1, s2=s2, rs=rs,
                ag=np.abs(g).sum(1, keepdims=True), agx=np.abs(g * xh).sum(1, keepdims=True), adg=np.abs(dy * xh).sum(0), adb=np.abs(dy).sum(0))


def bwd_bounds(ref, geo: Geo, bf16: bool):
    """dict(dx, dx_copy, dgamma, dbeta) of bounds."""
    L = int(math.log2(geo.lpr))
    b1 = (geo.nv + L + 6) * U * ref["ag"] / geo.dim
    b2 = (geo.nv + L + 9) * U * ref["agx"] / geo.dim
    xs2 = np.abs(ref["xh"] * ref["s2"])
    bdx = np.abs(ref["rs"]) * (4.0 * U * np.abs(ref["g"]) + 3.0 * U * np.abs(ref["s1"]) + 5.0 * U * xs2 + b1 + np.abs(ref["xh"]) * b2)
    if ref["res"] is not None:
        bdx = bdx + U * (np.abs(ref["dxc"]) + np.abs(ref["res"]))
    bdx = SECOND * bdx
    tail = geo.bwd_trips + 4 * geo.rpw + geo.sp_strided + SP_LANES
    return dict(dx=bdx, dx_copy=bdx + UB * (np.abs(ref["dx"]) + bdx) if bf16 else bdx, dgamma=SECOND * (3 + tail) * U * ref["adg"],
                dbeta=SECOND * tail * U * ref["adb"])


def rsqrt_eps_window(eps=EPS):
    """(value, allowed distance) of rstd for a constant row: var + eps = eps exactly, so only rsqrtf's own error remains."""
    r = 1.0 / math.sqrt(f32(eps))
    return r, RSQRT_ULP * float(np.spacing(F(r)))


# ------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    dtype: str        # "fp32" | "bf16": type of y, branch, dy and dx_copy
    rows: int
    dim: int
    add: bool         # forward with the fused residual add
    map: bool         # a row map: a strict subset of the full matrix in shuffled order
    accumulate: int   # backward adds into dx
    copy: bool        # backward writes dx_copy
    kind: str         # "table" | "fwd_wrap" | "bwd_wrap"

    @property
    def id(self) -> str:
        return f"{self.dtype}-{self.rows}x{self.dim}-{'add' if self.add else 'ln'}-{'map' if self.map else 'all'}-acc{self.accumulate}-{'copy' if self.copy else 'nocopy'}"

    @property
    def geo(self) -> Geo:
        return geometry(self.rows, self.dim)

    @property
    def src_rows(self) -> int:
        return self.rows + self.rows // 2 + 3 if self.map else self.rows

    @property
    def label(self) -> str:
        """The forward instantiation <T, NV, ADD, LPR>; the backward's is the same without ADD."""
        g = self.geo
        return f"<{self.dtype}, NV {g.nv}, ADD {int(self.add)}, LPR {g.lpr}>"


def row_counts(rpw: int):
    """(rows, add, map, accumulate, copy): 1, R - 1, 4R (one block), 4R + 1, 33 backward blocks with the last partly filled, 1001."""
    out = [(1, False, False, 1, True)]
    if rpw > 1:
        out.append((rpw - 1, True, False, 0, False))
    out += [(4 * rpw, False, True, 0, True), (4 * rpw + 1, True, True, 1, True), (32 * 4 * rpw + rpw + 1, None, False, 1, False), (1001, True, True, 0, True)]
    return out


FWD_WRAPS = [(32773, 196, True, False), (65539, 68, False, True), (131081, 8, True, True)]       # rows, dim, add, map
BWD_WRAPS = [(4097, 512, False, True), (8195, 384, True, False), (16389, 192, False, True)]


def cases():
    out = []
    for dtype in ("fp32", "bf16"):
        for lpr, nv, lo, hi in PAIRS:
            for dim in (lo, hi):
                for rows, add, mp, acc, cp in row_counts(64 // lpr):
                    out.append(Case(dtype, rows, dim, dim == hi if add is None else add, mp, acc, cp, "table"))
        for rows, dim, add, mp in FWD_WRAPS:
            out.append(Case(dtype, rows, dim, add, mp, 1, False, "fwd_wrap"))
        for rows, dim, add, mp in BWD_WRAPS:
            out.append(Case(dtype, rows, dim, add, mp, 0 if mp else 1, True, "bwd_wrap"))   # map + copy + accumulate 0: the engine's form
    return out


def coverage_gaps(cs) -> list:
    """What the issue's list asks for and ``cs`` does not reach; empty for cases()."""
    gaps = []
    for dtype in ("fp32", "bf16"):
        mine = [c for c in cs if c.dtype == dtype]
        for lpr, nv, lo, hi in PAIRS:
            R = 64 // lpr
            for dim in (lo, hi):
                at = [c for c in mine if c.dim == dim]
                if any((c.geo.lpr, c.geo.nv) != (lpr, nv) for c in at):
                    gaps.append(f"{dtype} dim {dim} does not select ({lpr}, {nv})")
                want = {1, 4 * R, 4 * R + 1} | ({R - 1} if R > 1 else set())
                have = {c.rows for c in at}
                for r in sorted(want - have):
                    gaps.append(f"{dtype} dim {dim}: no case with {r} rows")
                if not any(c.geo.bwd_grid == 33 and c.rows % (4 * R) != 0 for c in at):
                    gaps.append(f"{dtype} dim {dim}: no backward of 33 blocks with a partly filled last block")
                if not any(c.rows % 2 == 1 and 900 <= c.rows <= 1100 for c in at):
                    gaps.append(f"{dtype} dim {dim}: no odd row count near 1000")
            for add in (False, True):
                if not any((c.geo.lpr, c.geo.nv, c.add) == (lpr, nv, add) for c in mine):
                    gaps.append(f"{dtype}: forward <NV {nv}, ADD {int(add)}, LPR {lpr}> not launched")
        for lpr in (64, 32, 16):
            if not any(c.geo.lpr == lpr and c.geo.fwd_trips > 1 for c in mine):
                gaps.append(f"{dtype}: no forward wrap at {lpr} lanes per row")
            if not any(c.geo.lpr == lpr and c.geo.bwd_trips > 1 and c.geo.fwd_trips == 1 for c in mine):
                gaps.append(f"{dtype}: no backward-only wrap at {lpr} lanes per row")
        for what, pred in (("fused add with a row map", lambda c: c.add and c.map), ("fused add without a row map", lambda c: c.add and not c.map),
                           ("backward with row map + dx_copy + accumulate 0", lambda c: c.map and c.copy and c.accumulate == 0),
                           ("backward without a row map, accumulate 1", lambda c: not c.map and c.accumulate == 1)):
            if not any(pred(c) for c in mine):
                gaps.append(f"{dtype}: no {what}")
        if any(c.map and c.src_rows <= c.rows for c in mine):
            gaps.append(f"{dtype}: a row map that is no strict subset")
    return gaps


# ------------------------------------------------------------------------------------------------ data
def const_value(dim: int) -> float:
    """The value of the constant row whose y must equal beta bit for bit.  The compiler may contract v - sum * inv_d into one fma
    (it does in the NV = 1 kernels), which leaves c - c dim fl(1 / dim) instead of 0 unless dim fl(1 / dim) = 1 exactly.  So the row holds 3 at
    a power-of-two dim and 0 elsewhere: the only values that are exact with and without the contraction.  A second constant row of 3
    (row kind 3) is judged by its bound at every dim."""
    return 3.0 if is_pow2(dim) else 0.0


CONST_BOUNDED = 3.0


def row_kinds(rows: int) -> np.ndarray:
    """0 ordinary, 1 large mean, 2 constant (exact), 3 constant (bounded), per compact row.  rows = 1: ordinary; rows = 2: constant, large;
    else row 2 is the exact constant row, every fifth row from row 1 has the large mean, row 3 of more than four is the bounded constant row
    and the last row of more than three is ordinary."""
    k = np.zeros(rows, dtype=np.int64)
    if rows == 2:
        k[:] = (2, 1)
    elif rows > 2:
        k[1::5] = 1
        k[2] = 2
        if rows > 3:
            k[-1] = 0
        if rows > 4:
            k[3] = 3
    return k


def _seed(c: Case, salt: int):
    return [zlib.crc32(c.id.encode()), salt]


def _round(a, dtype):
    return to_bf16(a) if dtype == "bf16" else np.asarray(a, dtype=F)


def gen_case(c: Case):
    """The inputs of one case: dict(x, branch | None, gamma, beta, row_map | None, dy, res, kinds, const) as fp32 arrays (branch and dy hold
    bf16 values for a bf16 case).  x, branch and res have src_rows rows, dy has rows."""
    r = np.random.default_rng(_seed(c, 1))
    n, rows, dim = c.src_rows, c.rows, c.dim
    rmap = r.permutation(n)[:rows].astype(np.int32) if c.map else None
    src = _src(rows, rmap)
    kinds, cv = row_kinds(rows), const_value(dim)
    v = r.standard_normal((n, dim)) * 2.0 + 0.3
    big = src[kinds == 1]
    v[big] = 100.0 + 0.01 * r.standard_normal((big.size, dim))
    v[src[kinds == 2]] = cv
    v[src[kinds == 3]] = CONST_BOUNDED
    branch = None
    if c.add:
        branch = _round(r.standard_normal((n, dim)) * 0.5, c.dtype)
        flat = src[kinds >= 2]
        branch[flat] = _round(r.integers(-2, 3, (flat.size, dim)), c.dtype)
        v = v - _d(branch)
    return dict(x=v.astype(F), branch=branch, gamma=r.standard_normal(dim).astype(F), beta=r.standard_normal(dim).astype(F), row_map=rmap,
                dy=_round(r.standard_normal((rows, dim)), c.dtype), res=r.standard_normal((n, dim)).astype(F), kinds=kinds, const=cv)


def gen_exact(c: Case):
    """Inputs whose every fp32 intermediate is exact: small-integer x, dy, gamma and residual, mean 0, rstd 1/2 or 2 by row parity.  dgamma
    and dbeta are sums of integers below 2^24 at every dim; at a power-of-two dim s1, s2 and dx are exact as well, and so is the forward mean
    of x.  dict(x, gamma, beta, row_map, dy, res, mean, rstd, branch)."""
    r = np.random.default_rng(_seed(c, 2))
    n, rows, dim = c.src_rows, c.rows, c.dim
    rmap = r.permutation(n)[:rows].astype(np.int32) if c.map else None
    gam = r.integers(1, 3, dim) * r.choice([-1, 1], dim)
    return dict(x=r.integers(-4, 5, (n, dim)).astype(F), gamma=gam.astype(F), beta=r.integers(-3, 4, dim).astype(F), row_map=rmap,
                dy=r.integers(-3, 4, (rows, dim)).astype(F), res=r.integers(-5, 6, (n, dim)).astype(F), mean=np.zeros(rows, F),
                rstd=np.where(np.arange(rows) % 2 == 0, 0.5, 2.0).astype(F), branch=r.integers(-2, 3, (n, dim)).astype(F) if c.add else None)


def is_pow2(n: int) -> bool:
    return n & (n - 1) == 0


# ------------------------------------------------------------------------------------------------ comparison
def worst(out, ref, bound):
    """(worst error / bound, flat index of it); an element that is not finite, or off where the bound is zero, counts as infinite."""
    err = np.abs(_d(out) - ref)
    bound = np.broadcast_to(bound, err.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    ratio = np.where(np.isfinite(err), ratio, np.inf)
    i = int(np.argmax(ratio))
    return float(ratio.reshape(-1)[i]), i


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def _outside(n: int, src) -> np.ndarray:
    m = np.ones(n, dtype=bool)
    m[src] = False
    return m


def bwd_stats(c: Case, d, eps=EPS):
    """(mean, rstd) the backward of case ``c`` is given: the float64 statistics of the forward input rounded to fp32."""
    ref = fwd_ref(d["x"], d["gamma"], d["beta"], c.rows, d["row_map"], d["branch"], eps)
    return ref["mean"].astype(F), ref["rstd"].astype(F)


def check_fwd(c: Case, d, out, init_x_out=None, eps=EPS):
    """Every check of one forward launch.  out: dict(y (rows, dim), mean, rstd, x_out (src_rows, dim) | None) as fp32 arrays (bf16 widened).
    -> (ratios {output: worst error / bound}, failures [str]): bounds per element, x_out bit for bit on the mapped rows and untouched
    elsewhere (``init_x_out``: what it held before), the constant row's y = beta and rstd = rsqrt(eps)."""
    geo, src = c.geo, _src(c.rows, d["row_map"])
    ref = fwd_ref(d["x"], d["gamma"], d["beta"], c.rows, d["row_map"], d["branch"], eps)
    b = fwd_bounds(ref, geo, d["gamma"], d["beta"], c.dtype == "bf16", eps)
    ratios, fails = {}, []
    for name in ("mean", "rstd", "y"):
        ratio, i = worst(out[name], ref[name], b[name])
        ratios[name] = ratio
        if not ratio <= 1.0:
            r, col = (i, 0) if name != "y" else divmod(i, c.dim)
            fails.append(f"{name}: error / bound {ratio:.3g} (got {np.asarray(out[name]).reshape(-1)[i]!r}, fp64 {ref[name].reshape(-1)[i]!r}, bound "
                         f"{np.broadcast_to(b[name], ref[name].shape).reshape(-1)[i]:.3g}) at {locate(geo, r, col, False)}")
    if c.add:
        xo = out["x_out"]
        bad = np.argwhere(_bits(xo[src]) != _bits(ref["x_out"]))
        if bad.size:
            fails.append(f"x_out differs from fl32(x + branch) in {len(bad)} elements, first at {locate(geo, int(bad[0][0]), int(bad[0][1]), False)}")
        rest = _outside(c.src_rows, src)
        if init_x_out is not None and not np.array_equal(_bits(xo[rest]), _bits(init_x_out[rest])):
            fails.append("x_out: a row outside the map was written")
    for r in np.flatnonzero(d["kinds"] == 2):
        if not np.array_equal(_bits(out["y"][r]), _bits(_round(d["beta"], c.dtype))):
            fails.append(f"constant row {r}: y != beta ({locate(geo, int(r), 0, False)})")
        want, win = rsqrt_eps_window(eps)
        if not abs(float(out["rstd"][r]) - want) <= win:
            fails.append(f"constant row {r}: rstd {out['rstd'][r]!r} is not rsqrt(eps) = {want!r} within {RSQRT_ULP} ulp")
    return ratios, fails


def check_bwd(c: Case, d, mean, rstd, out, init_dx, exact=False):
    """Every check of one backward launch.  out: dict(dx (src_rows, dim), dx_copy | None, dgamma, dbeta); init_dx: dx before the launch.
    exact = the gen_exact data: dgamma and dbeta (every dim), dx and dx_copy (power-of-two dims) must equal the float64 values (dx_copy: their
    bf16 rounding) bit for bit instead of lying inside the bounds."""
    geo, src = c.geo, _src(c.rows, d["row_map"])
    ref = bwd_ref(d["dy"], d["x"], d["gamma"], mean, rstd, c.rows, d["row_map"], c.accumulate, d["res"])
    b = bwd_bounds(ref, geo, c.dtype == "bf16")
    ratios, fails = {}, []
    got = dict(dx=out["dx"][src], dgamma=out["dgamma"], dbeta=out["dbeta"])
    if c.copy:
        got["dx_copy"] = out["dx_copy"][src]
        ref["dx_copy"] = ref["dx"]
    for name, val in got.items():
        per_row = name in ("dx", "dx_copy")
        if exact and (not per_row or is_pow2(c.dim)):
            want = ref[name].astype(F)
            if name == "dx_copy":
                want = _round(want, c.dtype)
            bad = np.flatnonzero((_bits(val) != _bits(want)).reshape(-1))
            ratios[name] = 0.0 if not bad.size else math.inf
            if bad.size:
                i = int(bad[0])
                where = locate(geo, *divmod(i, c.dim), True) if per_row else locate_col(geo, i, name == "dbeta")
                fails.append(f"{name}: {bad.size} elements differ from the exact value, first got {val.reshape(-1)[i]!r} want {want.reshape(-1)[i]!r} at {where}")
            continue
        if exact:
            continue
        ratio, i = worst(val, ref[name], b[name])
        ratios[name] = ratio
        if not ratio <= 1.0:
            where = locate(geo, *divmod(i, c.dim), True) if per_row else locate_col(geo, i, name == "dbeta")
            fails.append(f"{name}: error / bound {ratio:.3g} (got {np.asarray(val).reshape(-1)[i]!r}, fp64 {ref[name].reshape(-1)[i]!r}, bound {b[name].reshape(-1)[i]:.3g}) at {where}")
    rest = _outside(c.src_rows, src)
    if not np.array_equal(_bits(out["dx"][rest]), _bits(init_dx[rest])):
        fails.append("dx: a row outside the map was written")
    if c.copy and not np.all(np.isnan(out["dx_copy"][rest])):
        fails.append("dx_copy: a row outside the map was written")
    return ratios, fails


def check_exact_fwd(c: Case, d, out):
    """gen_exact data through the forward: x_out = fl32(x + branch) bit for bit, and at a power-of-two dim the mean equals the float64 mean."""
    src = _src(c.rows, d["row_map"])
    ref = fwd_ref(d["x"], d["gamma"], d["beta"], c.rows, d["row_map"], d["branch"])
    fails = []
    if c.add and not np.array_equal(_bits(out["x_out"][src]), _bits(ref["x_out"])):
        fails.append("x_out differs from fl32(x + branch)")
    if is_pow2(c.dim):
        bad = np.flatnonzero(_bits(out["mean"]) != _bits(ref["mean"].astype(F)))
        if bad.size:
            fails.append(f"mean of integer rows is not exact, first at {locate(c.geo, int(bad[0]), 0, False)}")
    return fails
