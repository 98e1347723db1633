"""numpy restatement of the kernels only the engine launches, for the tests: full_grad_split / patch_grad_split and
zero_token_rows (k_classifier.hip), features_pool (k_representation.hip), cast, add_rows_pos, add_into (k_patch.hip) and
linear_dgrad on the tiled fp32 kernel (k_gemm.hip), reached one by one through mae_full_grad_split, mae_zero_token_rows,
mae_features_pool, mae_cast, mae_add_rows_pos, mae_add_into and mae_linear_dgrad.

numpy on the CPU: no torch, no GPU.  The buffers, Exact / Bounded / Scratch and ``judge`` are token_ref's; the bf16 rounding is
optim_ref's; the LayerNorm bound and the geometry of sum_partials are ln_ref's.  Per kernel there is a case table, ``gen_*`` (the
inputs), ``*_inits`` (the NaN-filled output buffers with guard rows), ``expect_*`` (output name -> Exact | Bounded | Scratch) and
``simulate_*``: the plain fp32 numpy evaluation in the kernel's own order, which takes a ``mutate`` name and then restates one
specific way of getting the kernel wrong (the host test requires every mutant to fail).

Exact (integer views over the whole buffer, guard rows included):
  dtok            a copy of dx, or its bf16 rounding (nearest even); with a class token row 0 of every image is +0.0.
  dcls            with a class token the launcher copies dpos[0]: equal bit for bit (``split_extra``); without one dcls and
                  dpos[0] are memset: +0.0.
  zero_token_rows +0.0 in the rows r % L != 0 of both buffers, every other row keeps its bits.
  cast            fp32 -> bf16 is optim_ref.bf16_rne (a NaN keeps its upper half, quiet), bf16 -> fp32 appends 16 zero bits, equal
                  types copy.  The patterns: quiet NaNs, +-inf, -0, the smallest and the largest denormal (fp32 ones round to
                  bf16 denormals or to the smallest normal), ties to even in both directions, the largest finite value (rounds
                  to inf).
  add_rows_pos    fl(x + pos[r % L]): numpy's float32 addition.
  add_into        fl(dst + src), or bf16_rne(fl(widen(dst) + src)); pairs whose fp32 sum is a bf16 tie are among the inputs.
  dpos on the integer inputs (|x| <= 8, sum|x| < 2^24): every partial sum is an integer fp32 holds, so any order returns the
                  float64 sum; a dropped or doubled image changes the integer.
  features_pool   kind const: every pooled row of x_mid + branch is a constant small integer c (branch integer, x_mid = c - branch).
                  The row sum c D is exact in any order, the division by (float)D returns c, v - mean = +0, so
                  y = 0 * rstd * gamma + beta = beta with or without contraction, and the pool of n equal rows of integer beta is
                  n beta / n = beta (IEEE division of an exactly divisible pair).  kind zero: the same with beta = 0 under L2:
                  f = +0 and out = 0 / (0 + 1e-8) = +0.

Bounded, u = 2^-24, SECOND = 1 + 2^-16 for the second order (ln_ref):
  dpos on random data       |err| <= c u sum_b|dx|,  c = ceil(B / S) + ceil(S / 32) + 32: a summand goes through at most
                  ceil(B / S) additions into its slice's accumulator (four rows in flight do not change the count), then
                  sum_partials (ln_ref: ceil(G / 32) strided additions of a row lane with G = S, and the 32 row lanes in order).
                  S = slices(B, L, D) restates full_grad_split_slices.  The first addition into each of the three zero
                  accumulators does not round; those three pay for the second-order terms, as in token_ref.
  features_pool   every normalised row by ln_ref.fwd_bounds with the geometry the kernel has: 64 lanes per row, 4 vectors per
                  lane whatever dim (absent ones add exact zeros).  Its counts cover this kernel's: the mean divides by
                  (float)dim (1 rounding where ln_ref counts 2), and rstd = 1 / sqrtf(.): sqrtf is correctly rounded under the
                  compiler's default, SQRT_ULP = 1 ulp = 2 u is allowed (not measured), the division adds u, 3 u in all against
                  ln_ref's RSQRT_ULP allowance of 4 u.  Then with n = hi - lo and by the row bounds:
                      pool   k = ceil(n / 4) + 3 + 1 (the wave's additions, the 3 wave additions, the division):
                             bf = SECOND (sum_t by + k u sum_t (|y| + by)) / n
                      L2     ss = sum f^2: the square 1, ((a + b) + (c + d)) 2, block_sum_256 6 + 3: 12 roundings of non-negative
                             terms; sqrtf halves them and adds SQRT_ULP, the addition of 1e-8 one more, the division one more:
                             rho = 6 u SECOND + 2 u SQRT_ULP + u,  dden = ||bf||_2 + rho den,  den = ||f||_2 + fl(1e-8),
                             |err| <= SECOND (bf / (den - dden) + |out| dden / (den - dden) + u |out|)
  linear_dgrad    fp32 accumulation: one fmaf chain over the N terms of an output in ascending order, so
                      e_acc = SECOND N u sum_n |dy w|
                  (gemm_ref.check_nt counts K / 32 + 2 roundings, one per 32-deep MFMA: that derivation does NOT hold for this
                  kernel, which rounds after every term, so the bound is derived here beside it).  The epilogue, with q the
                  factor and eq its error:  |err| <= SECOND (e_acc (|q| + eq) + |pre| eq + u |ref|), a bf16 output adds
                  2^-8 (|ref| + that).  NONE: q = 1, eq = 0 and no rounding.  MUL: q = aux, eq = 0.  DGELU: q = gelu_erf'(aux) =
                  cdf + aux pdf evaluated by the device in fp32 from erff and __expf; ROCm's accuracy table is not among the files of
                  an installation, so ERFF_ULP = 4 ulp and EXPF_ULP = 2 ulp are allowed (not measured).  With z = aux / sqrt 2,
                  t = -aux^2 / 2:
                      cdf    the argument fl(aux fl(1 / sqrt 2)) is off by 2 u |z|, erf' = 2 / sqrt(pi) exp(-z^2); erff 2 u ERFF_ULP |erf|;
                             1 + erf rounds once, the halving is exact:   ecdf = (2 u |z| erf'(z) + 2 u ERFF_ULP |erf z|) / 2 + u cdf
                      pdf    t = fl(fl(-0.5 aux) aux) is off by u |t|, __expf multiplies by log2 e (constant and product: 2 u |t| more)
                             and takes v_exp_f32; the constant 1 / sqrt(2 pi) and its product round twice:
                                                                          rpdf = 3 u |t| + 2 u EXPF_ULP + 2 u
                      q      aux pdf rounds once, the sum once:           eq = SECOND (ecdf + |aux| pdf (rpdf + u) + u |q|)
                  (|aux| < 8 in the cases: no term is near the denormal range.)
Bounds are evaluated from the inputs and the float64 reference only, never fitted to a kernel's output."""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from tests import ln_ref
from tests.ln_ref import SECOND, SP_LANES, UB
from tests.optim_ref import bf16_rne
from tests.token_ref import GUARD, U, Bounded, Exact, Scratch, _seed, bits, cdiv, from_dt, judge, nan_buf, to_dt  # noqa: F401 (re-exported)

F = np.float32
EMBED_SLICES = 64             # CLS_EMBED_SLICES
SLICE_BLOCKS = 2048           # blocks one full_grad_split launch may have
ZERO_BLOCKS = 8192            # zero_token_rows
ELEM_BLOCKS = 256 * 16        # cast, add_into, add_rows_pos: grid-stride over 256 * ELEM_BLOCKS threads
ELEM_TRIP = 256 * ELEM_BLOCKS
TILE, TILE_K = 64, 16         # gemm_generic_kernel
SQRT_ULP, ERFF_ULP, EXPF_ULP = 1, 4, 2
EPS = 1e-6
NONE, DGELU, MUL = 0, 3, 5    # MAE_EPI_*
KERNELS = ("full_grad_split", "zero_token_rows", "features_pool", "cast", "add_rows_pos", "add_into", "linear_dgrad")


def widen(a) -> np.ndarray:
    """fp32 values of a float32 or bf16-pattern array, NaN patterns kept (the upper half)."""
    return from_dt(np.ascontiguousarray(a))


def bf16_trunc(x32) -> np.ndarray:
    return (np.ascontiguousarray(x32, dtype=F).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _fill(init: np.ndarray, val: np.ndarray) -> np.ndarray:
    out = init.copy()
    v = np.asarray(val).reshape((-1,) + init.shape[1:])
    assert v.dtype == init.dtype, (v.dtype, init.dtype)
    out[:len(v)] = v
    return out


# ------------------------------------------------------------------------------------------------ full_grad_split
def slices(B: int, L: int, D: int) -> int:
    """full_grad_split_slices: batch slices of one launch."""
    per_slice = cdiv(L * (D // 4), 256)
    return max(1, min(B, EMBED_SLICES, cdiv(SLICE_BLOCKS, per_slice)))


def slice_bounds(B: int, S: int):
    return [(B * s // S, B * (s + 1) // S) for s in range(S)]


@dataclass(frozen=True)
class SplitCase:
    id: str
    B: int
    L: int          # rows per image (with_cls = 0: patch rows)
    D: int
    S: int          # the slice count the case is meant to reach
    with_cls: bool
    dtype: str

    @property
    def pos_rows(self):
        return self.L if self.with_cls else self.L + 1


# (B, L, D, S): one thread; slices of one image + the u tail; 816 threads = a partial fourth block; S = 64 with slices of 1 and 2
# images; slices of 4 and 5; the cdiv(2048, per_slice) limit; several blocks per slice with a ragged last one
SPLIT_SHAPES = ((1, 1, 4, 1), (3, 5, 8, 3), (5, 17, 192, 5), (67, 17, 192, 64), (300, 3, 1024, 64), (60, 50, 768, 54), (9, 145, 384, 9))


def split_cases():
    return [SplitCase(f"B{B}L{L}D{D}-{'cls' if w else 'patch'}-{dt}", B, L, D, S, w, dt)
            for B, L, D, S in SPLIT_SHAPES for w in (True, False) for dt in ("f32", "bf16")]


def gen_split(c: SplitCase, exact: bool = False) -> dict:
    rng = np.random.default_rng(_seed(c.id) + exact)
    shape = (c.B, c.L, c.D)
    dx = rng.integers(-8, 9, size=shape).astype(F) if exact else rng.standard_normal(shape, dtype=F)
    return dict(dx=dx)


def split_inits(c: SplitCase) -> dict:
    return {"full_grad_split.dtok": nan_buf(c.B * c.L, c.D, c.dtype), "full_grad_split.dpos": nan_buf(c.pos_rows, c.D),
            "full_grad_split.dcls": nan_buf(c.D, 0), "full_grad_split.partial": nan_buf(slices(c.B, c.L, c.D) * c.L * c.D, 0)}


def split_chain(c: SplitCase) -> int:
    S = slices(c.B, c.L, c.D)
    return cdiv(c.B, S) + cdiv(S, SP_LANES) + SP_LANES


def expect_split(c: SplitCase, d: dict, exact: bool = False) -> dict:
    dx = d["dx"]
    dtok = dx.copy()
    if c.with_cls:
        dtok[:, 0] = 0.0
    ref = dx.astype(np.float64).sum(0)                                   # (L, D)
    mag = np.abs(dx).astype(np.float64).sum(0)
    head = np.zeros((c.pos_rows - c.L, c.D))                             # the memset row of the patch-only variant
    if exact:
        assert np.all(dx == np.rint(dx)) and np.abs(dx).max() <= 8 and mag.max() < 2.0 ** 24
        dpos = Exact(np.concatenate([head, ref]).astype(F))
        dcls = Exact(ref[0].astype(F) if c.with_cls else np.zeros(c.D, F))
    else:
        bound = split_chain(c) * U * mag
        dpos = Bounded(np.concatenate([head, ref]), np.concatenate([head, bound]))
        dcls = Bounded(ref[0], bound[0]) if c.with_cls else Exact(np.zeros(c.D, F))
    return {"full_grad_split.dtok": Exact(to_dt(dtok.reshape(-1, c.D), c.dtype)), "full_grad_split.dpos": dpos, "full_grad_split.dcls": dcls,
            "full_grad_split.partial": Scratch(slices(c.B, c.L, c.D) * c.L * c.D)}


def sum_partials(partial: np.ndarray) -> np.ndarray:
    """sum_partials_kernel on partial (G, C) fp32: row lane rl adds rows rl, rl + 32, .. in order, then the 32 row lanes in order."""
    G = partial.shape[0]
    red = np.zeros((SP_LANES,) + partial.shape[1:], F)
    for i in range(G):
        red[i % SP_LANES] = red[i % SP_LANES] + partial[i]
    v = np.zeros(partial.shape[1:], F)
    for j in range(SP_LANES):
        v = v + red[j]
    return v


def simulate_split(c: SplitCase, d: dict, mutate: str = "") -> dict:
    """mutate: slice_off_by_one (a slice ends one image early) | drop_u_tail (the last, partial group of four images of a slice is
    skipped) | copy_cls_row (dtok keeps the class row) | dcls_row1."""
    dx, S = d["dx"], slices(c.B, c.L, c.D)
    dtok = np.full_like(dx, np.nan)
    partial = np.zeros((S, c.L, c.D), F)
    for s, (b0, b1) in enumerate(slice_bounds(c.B, S)):
        if mutate == "slice_off_by_one" and s < S - 1:
            b1 -= 1
        if mutate == "drop_u_tail":
            b1 = b0 + (b1 - b0) // 4 * 4
        for b in range(b0, b1):
            partial[s] = partial[s] + dx[b]
            dtok[b] = dx[b]
            if c.with_cls and mutate != "copy_cls_row":
                dtok[b, 0] = 0.0
    total = sum_partials(partial)
    dpos = np.concatenate([np.zeros((c.pos_rows - c.L, c.D), F), total])
    dcls = dpos[1 if mutate == "dcls_row1" and c.L > 1 else 0].copy() if c.with_cls else np.zeros(c.D, F)
    init = split_inits(c)
    out = {"full_grad_split.dpos": _fill(init["full_grad_split.dpos"], dpos), "full_grad_split.dcls": _fill(init["full_grad_split.dcls"], dcls),
           "full_grad_split.partial": _fill(init["full_grad_split.partial"], partial.reshape(-1))}
    tok = init["full_grad_split.dtok"]
    written = ~np.isnan(dtok.reshape(-1, c.D)[:, 0])                    # dx holds no NaN: an image the mutant skipped stays unwritten
    tok[:c.B * c.L][written] = to_dt(dtok.reshape(-1, c.D), c.dtype)[written]
    out["full_grad_split.dtok"] = tok
    return out


def split_extra(c: SplitCase, got: dict) -> list:
    """What an Exact | Bounded table cannot say: dcls is the copy of dpos[0]; the memset rows are +0.0."""
    dpos, dcls = got["full_grad_split.dpos"], got["full_grad_split.dcls"]
    if c.with_cls:
        return [] if np.array_equal(bits(dpos[0]), bits(dcls[:c.D])) else ["full_grad_split.dcls: not the bits of dpos[0]"]
    return [] if not bits(dpos[0]).any() else ["full_grad_split.dpos: row 0 of the patch-only variant is not +0.0"]


# ------------------------------------------------------------------------------------------------ zero_token_rows
@dataclass(frozen=True)
class ZeroCase:
    id: str
    rows: int
    L: int
    D: int
    dtype: str


def zero_rpb(D: int) -> int:
    return 4 if D // 4 <= 64 else 2


def zero_cases():
    """D 8 and 256 (64 lanes, D4 = 64 exactly), 260 (128 lanes, 65 of them busy), 1024 (two passes of 128 lanes); L = 1 (every row
    is a class row: nothing may change) and 5 with 23 rows (no multiple of 5); second grid trips of both lane splits."""
    out = [ZeroCase(f"D{D}-L{L}-{dt}", 23, L, D, dt) for D in (8, 256, 260, 1024) for L in (1, 5) for dt in ("f32", "bf16")]
    out += [ZeroCase("D8-trip-f32", ZERO_BLOCKS * 4 + 3, 5, 8, "f32"), ZeroCase("D8-trip-bf16", ZERO_BLOCKS * 4 + 3, 5, 8, "bf16"),
            ZeroCase("D260-trip-bf16", ZERO_BLOCKS * 2 + 3, 7, 260, "bf16")]
    return out


def gen_zero(c: ZeroCase) -> dict:
    rng = np.random.default_rng(_seed(c.id))
    return dict(dres=rng.standard_normal((c.rows, c.D), dtype=F), dres_c=to_dt(rng.standard_normal((c.rows, c.D), dtype=F), c.dtype))


def zero_inits(c: ZeroCase, d: dict) -> dict:
    return {"zero_token_rows.dres": _fill(nan_buf(c.rows, c.D), d["dres"]), "zero_token_rows.dres_c": _fill(nan_buf(c.rows, c.D, c.dtype), d["dres_c"])}


def simulate_zero(c: ZeroCase, d: dict, mutate: str = "") -> dict:
    """mutate: mod_L_plus_1 | no_last_trip (rows past the first grid trip keep their values) | one_lane_pass (columns past 128 float4
    lanes are not cleared)."""
    r = np.arange(c.rows)
    clear = r % (c.L + 1 if mutate == "mod_L_plus_1" else c.L) != 0
    if mutate == "no_last_trip":
        clear &= r < ZERO_BLOCKS * zero_rpb(c.D)
    cols = min(c.D, 512) if mutate == "one_lane_pass" else c.D
    a, b = d["dres"].copy(), d["dres_c"].copy()
    a[clear, :cols], b[clear, :cols] = 0, 0
    init = zero_inits(c, d)
    return {"zero_token_rows.dres": _fill(init["zero_token_rows.dres"], a), "zero_token_rows.dres_c": _fill(init["zero_token_rows.dres_c"], b)}


def expect_zero(c: ZeroCase, d: dict) -> dict:
    clear = np.arange(c.rows) % c.L != 0
    a, b = d["dres"].copy(), d["dres_c"].copy()
    a[clear], b[clear] = 0, 0
    return {"zero_token_rows.dres": Exact(a), "zero_token_rows.dres_c": Exact(b)}


# ------------------------------------------------------------------------------------------------ features_pool
@dataclass(frozen=True)
class PoolCase:
    id: str
    B: int
    seq: int
    D: int
    lo: int
    hi: int
    dtype: str      # of branch
    l2: bool
    kind: str       # random | const | zero

    @property
    def n(self):
        return self.hi - self.lo


POOL_DIMS = (4, 8, 192, 256, 260, 768, 1024)        # D4 = 1, 2, 48, 64 (one full pass), 65 (lane 0 owns two vectors), 192, 256 (every lane four)
POOL_RANGES = ((1, 0, 1), (10, 0, 1), (10, 1, 10), (10, 0, 10), (10, 1, 3), (10, 1, 4), (10, 2, 6), (10, 1, 6), (10, 1, 9))   # (seq, lo, hi)


def pool_cases():
    """hi - lo in 1 .. 5, 8, 9, 10: below 4 some waves own no row, 5 and 9 give wave 0 one row more; seq = 1; the class row alone,
    the patch rows, the whole sequence.  Every dim with both branch types and both normalisations on random data; the exact kinds
    at three row counts per dim."""
    out = []
    for D in POOL_DIMS:
        for seq, lo, hi in POOL_RANGES:
            for dt in ("f32", "bf16"):
                for l2 in (False, True):
                    out.append(PoolCase(f"D{D}-s{seq}r{lo}_{hi}-{dt}-{'l2' if l2 else 'none'}", 3, seq, D, lo, hi, dt, l2, "random"))
        for seq, lo, hi in ((1, 0, 1), (10, 1, 4), (10, 1, 10)):
            out.append(PoolCase(f"D{D}-s{seq}r{lo}_{hi}-const", 3, seq, D, lo, hi, "bf16" if hi == 4 else "f32", False, "const"))
            out.append(PoolCase(f"D{D}-s{seq}r{lo}_{hi}-zero", 3, seq, D, lo, hi, "f32" if hi == 4 else "bf16", True, "zero"))
    return out


def gen_pool(c: PoolCase) -> dict:
    """x_mid, branch (B, seq, D); rows outside [lo, hi) hold NaN: the kernel reads the pooled rows only."""
    rng = np.random.default_rng(_seed(c.id))
    shape = (c.B, c.seq, c.D)
    if c.kind == "random":
        branch = to_dt(rng.standard_normal(shape, dtype=F) * F(0.5), c.dtype)
        x = (rng.standard_normal(shape, dtype=F) * F(2.0) + F(0.3)).astype(F)
        gamma, beta = rng.standard_normal(c.D, dtype=F), rng.standard_normal(c.D, dtype=F)
    else:
        b32 = rng.integers(-2, 3, size=shape).astype(F)
        branch = to_dt(b32, c.dtype)
        x = (rng.integers(-3, 4, size=(c.B, c.seq, 1)).astype(F) - b32).astype(F)
        gamma = rng.standard_normal(c.D, dtype=F)
        beta = rng.integers(-3, 4, size=c.D).astype(F) if c.kind == "const" else np.zeros(c.D, F)
    out_rows = np.ones(c.seq, bool)
    out_rows[c.lo:c.hi] = False
    x[:, out_rows] = np.nan
    branch = branch.reshape(shape)
    branch[:, out_rows] = 0x7FC0 if c.dtype == "bf16" else np.nan
    return dict(x=x, branch=branch, gamma=gamma, beta=beta)


def pool_inits(c: PoolCase) -> dict:
    return {"features_pool.out": nan_buf(c.B, c.D)}


def pool_geo(D: int) -> ln_ref.Geo:
    """The LayerNorm geometry of features_kernel for ln_ref.fwd_bounds: a wave per row, four vectors per lane."""
    return ln_ref.Geo(rows=1, dim=D, lpr=64, nv=4, rpw=1, fwd_grid=1, bwd_grid=1, fwd_trips=1, bwd_trips=1, lds_floats=0, sp_blocks=0, sp_strided=0)


def expect_pool(c: PoolCase, d: dict) -> dict:
    if c.kind == "const":
        return {"features_pool.out": Exact(np.tile(d["beta"], (c.B, 1)))}
    if c.kind == "zero":
        return {"features_pool.out": Exact(np.zeros((c.B, c.D), F))}
    x = d["x"][:, c.lo:c.hi].reshape(-1, c.D)
    br = widen(d["branch"])[:, c.lo:c.hi].reshape(-1, c.D)
    ref = ln_ref.fwd_ref(x, d["gamma"], d["beta"], len(x), None, br, EPS)
    by = ln_ref.fwd_bounds(ref, pool_geo(c.D), d["gamma"], d["beta"], False, EPS)["y"].reshape(c.B, c.n, c.D)
    y = ref["y"].reshape(c.B, c.n, c.D)
    k = cdiv(c.n, 4) + 3 + 1
    f = y.sum(1) / c.n
    bf = SECOND * (by.sum(1) + k * U * (np.abs(y) + by).sum(1)) / c.n
    if not c.l2:
        return {"features_pool.out": Bounded(f, bf)}
    den = np.sqrt((f * f).sum(1, keepdims=True)) + float(F(1e-8))
    rho = 6 * U * SECOND + 2 * U * SQRT_ULP + U
    dden = np.sqrt((bf * bf).sum(1, keepdims=True)) + rho * den
    out = f / den
    assert np.all(dden < 0.5 * den)
    return {"features_pool.out": Bounded(out, SECOND * (bf / (den - dden) + np.abs(out) * dden / (den - dden) + U * np.abs(out)))}


def _wave_sum(s: np.ndarray) -> np.ndarray:
    """wave_sum over the last axis (64 lanes): the xor butterfly 32, 16, .. 1; every lane ends with the same value."""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[..., lane ^ o]
    return s


def simulate_pool(c: PoolCase, d: dict, mutate: str = "") -> dict:
    """mutate: divide_by_seq | skip_last_column (float4 column D4 - 1 is left out of the row statistics) | waves_of_three (rows
    lo + 3, lo + 7, .. are never added)."""
    D4 = c.D // 4
    x = d["x"][:, c.lo:c.hi]
    v = np.zeros((c.B, c.n, 1024), F)
    v[..., :c.D] = x + widen(d["branch"])[:, c.lo:c.hi]                  # fl32(x_mid + branch); absent columns are exact zeros
    q4 = v.reshape(c.B, c.n, 4, 64, 4)                                   # [.., i, lane, 4]: float4 column lane + 64 i
    have = (np.arange(64)[None, :] + 64 * np.arange(4)[:, None]) < (D4 - (mutate == "skip_last_column"))   # (i, lane)
    s = np.zeros((c.B, c.n, 64), F)
    for i in range(4):
        t = (q4[:, :, i, :, 0] + q4[:, :, i, :, 1]) + (q4[:, :, i, :, 2] + q4[:, :, i, :, 3])
        s = s + np.where(have[i], t, F(0))
    mean = _wave_sum(s)[..., :1] / F(c.D)                                # (B, n, 1)
    dv = q4 - mean[..., None, None]
    sq = np.zeros((c.B, c.n, 64), F)
    for i in range(4):
        e = dv[:, :, i]
        t = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + (e[..., 2] * e[..., 2] + e[..., 3] * e[..., 3])
        sq = sq + np.where(have[i], t, F(0))
    rstd = F(1.0) / np.sqrt(_wave_sum(sq)[..., :1] / F(c.D) + F(EPS))
    dvf = (v[..., :c.D] - mean)
    y = dvf * rstd * d["gamma"] + d["beta"]                              # (B, n, D) fp32, left to right
    acc = np.zeros((4, c.B, c.D), F)
    for j in range(c.n):
        if mutate == "waves_of_three" and j % 4 == 3:
            continue
        acc[j % 4] = acc[j % 4] + y[:, j]
    f = acc[0]
    for w in range(1, 4):
        f = f + acc[w]
    f = f / F(c.seq if mutate == "divide_by_seq" else c.n)
    if c.l2:
        fp = np.zeros((c.B, 1024), F)
        fp[:, :c.D] = f
        g = fp.reshape(c.B, 256, 4)
        th = (g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + (g[..., 2] * g[..., 2] + g[..., 3] * g[..., 3])   # per thread
        w = _wave_sum(th.reshape(c.B, 4, 64))[..., 0]
        ss = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
        f = f / (np.sqrt(ss) + F(1e-8))[:, None]
    assert f.dtype == F
    return {"features_pool.out": _fill(pool_inits(c)["features_pool.out"], f)}


# ------------------------------------------------------------------------------------------------ cast, add_into
@dataclass(frozen=True)
class ElemCase:
    id: str
    n: int


def elem_cases():
    """One thread; a part-filled block; a block and one thread; 256 * 4096 threads and three more elements: the second grid trip."""
    return [ElemCase(f"n{n}", n) for n in (1, 255, 257, ELEM_TRIP + 3)]


# fp32 patterns: quiet NaNs, infinities, zeros, smallest / largest denormal, a denormal that is a bf16 denormal tie, the largest finite
# value (rounds to inf in bf16), ties to even downwards (1 + 2^-8) and upwards (1 + 3 2^-8), just above and just below a tie
CAST_F32 = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800000, 0xFF800000, 0x80000000, 0x00000000, 0x00000001, 0x807FFFFF, 0x00018000,
                     0x00008000, 0x7F7FFFFF, 0x3F808000, 0x3F818000, 0x3F808001, 0x3F817FFF, 0xBF808000, 0x007F8000], np.uint32)
CAST_BF16 = np.array([0x7FC0, 0xFFC0, 0x7FC1, 0x7F80, 0xFF80, 0x8000, 0x0000, 0x0001, 0x807F, 0x0080, 0x7F7F, 0x3F80, 0xBF81], np.uint16)
DT_PAIRS = (("f32", "bf16"), ("bf16", "f32"), ("f32", "f32"), ("bf16", "bf16"))


def gen_cast(c: ElemCase, src: str) -> dict:
    """Random normal values with the special patterns in front (n = 1: a tie) and, past one grid trip, behind the trip as well."""
    rng = np.random.default_rng(_seed(c.id + src))
    x = to_dt(rng.standard_normal(c.n, dtype=F) * F(3.0), src)
    sp = CAST_F32.view(F) if src == "f32" else CAST_BF16
    if c.n == 1:
        sp = sp[13:14] if src == "f32" else sp[12:13]                   # the tie 1 + 3 2^-8, which truncation gets wrong (fp32); -1.0078125 (bf16)
    m = min(c.n, len(sp))
    x[:m] = sp[:m]
    if c.n > ELEM_TRIP:
        x[-3:] = sp[:3][::-1] if src == "bf16" else sp[12:15]
    return dict(src=x)


def cast_inits(c: ElemCase, dst: str) -> dict:
    return {"cast.dst": nan_buf(c.n, 0, dst)}


def _cast(x, src: str, dst: str, trunc: bool = False) -> np.ndarray:
    if src == dst:
        return x.copy()
    if dst == "f32":
        return widen(x).copy()
    return bf16_trunc(x) if trunc else bf16_rne(x)


def expect_cast(c: ElemCase, d: dict, src: str, dst: str) -> dict:
    return {"cast.dst": Exact(_cast(d["src"], src, dst))}


def simulate_cast(c: ElemCase, d: dict, src: str, dst: str, mutate: str = "") -> dict:
    """mutate: truncate | no_last_trip."""
    out = _cast(d["src"], src, dst, mutate == "truncate")
    full = cast_inits(c, dst)["cast.dst"]
    m = min(c.n, ELEM_TRIP) if mutate == "no_last_trip" else c.n
    full[:m] = out[:m]
    return {"cast.dst": full}


def gen_add_into(c: ElemCase, dtype: str) -> dict:
    """dst (dtype) and src (fp32): random values, with pairs in front (and behind one grid trip) whose fp32 sum is a bf16 tie: 1.0078125 + 2^-8
    (to even: up), 1 + 2^-8 (to even: down), their negatives, and a sum that rounds to fp32 first."""
    rng = np.random.default_rng(_seed(c.id + dtype))
    dst = rng.standard_normal(c.n, dtype=F)
    src = rng.standard_normal(c.n, dtype=F)
    pd = np.array([1.0078125, 1.0, -1.0078125, -1.0, 1.0, 256.0], F)
    ps = np.array([2.0 ** -8, 2.0 ** -8, -2.0 ** -8, -2.0 ** -8, 2.0 ** -8 + 2.0 ** -24, 1.0 + 2.0 ** -17], F)
    m = min(c.n, len(pd))
    dst[:m], src[:m] = pd[:m], ps[:m]
    if c.n > ELEM_TRIP:
        dst[-3:], src[-3:] = pd[:3], ps[:3]
    return dict(dst=to_dt(dst, dtype), src=src)


def add_into_inits(c: ElemCase, d: dict) -> dict:
    dt = "bf16" if d["dst"].dtype == np.uint16 else "f32"
    return {"add_into.dst": _fill(nan_buf(c.n, 0, dt), d["dst"])}


def _add_into(d: dict, trunc: bool = False) -> np.ndarray:
    s = (widen(d["dst"]) + d["src"]).astype(F)
    if d["dst"].dtype == np.uint16:
        return bf16_trunc(s) if trunc else bf16_rne(s)
    return s


def expect_add_into(c: ElemCase, d: dict) -> dict:
    return {"add_into.dst": Exact(_add_into(d))}


def simulate_add_into(c: ElemCase, d: dict, mutate: str = "") -> dict:
    """mutate: truncate | no_last_trip."""
    out = _add_into(d, mutate == "truncate")
    full = add_into_inits(c, d)["add_into.dst"]
    m = min(c.n, ELEM_TRIP) if mutate == "no_last_trip" else c.n
    full[:m] = out[:m]
    return {"add_into.dst": full}


# ------------------------------------------------------------------------------------------------ add_rows_pos
@dataclass(frozen=True)
class PosCase:
    id: str
    rows: int
    L: int
    D: int


def pos_cases():
    """One float4 per row with a ragged row count; rows = L; more than 256 * 4096 float4 (a second grid trip) with rows % L != 0."""
    return [PosCase(f"r{r}L{L}D{D}", r, L, D) for r, L, D in ((7, 3, 4), (10, 10, 192), (4100, 145, 1024))]


def gen_pos(c: PosCase) -> dict:
    rng = np.random.default_rng(_seed(c.id))
    return dict(x=rng.standard_normal((c.rows, c.D), dtype=F), pos=rng.standard_normal((c.L, c.D), dtype=F))


def pos_inits(c: PosCase) -> dict:
    return {"add_rows_pos.out": nan_buf(c.rows, c.D)}


def _rows_pos(c: PosCase, d: dict, mod: int) -> np.ndarray:
    return d["x"] + d["pos"][(np.arange(c.rows) % mod) % c.L]


def expect_pos(c: PosCase, d: dict) -> dict:
    return {"add_rows_pos.out": Exact(_rows_pos(c, d, c.L))}


def simulate_pos(c: PosCase, d: dict, mutate: str = "") -> dict:
    """mutate: mod_L_plus_1 | no_last_trip."""
    out = _rows_pos(c, d, c.L + 1 if mutate == "mod_L_plus_1" else c.L).reshape(-1)
    full = pos_inits(c)["add_rows_pos.out"]
    m = min(out.size, 4 * ELEM_TRIP) if mutate == "no_last_trip" else out.size
    full.reshape(-1)[:m] = out[:m]
    return {"add_rows_pos.out": full}


# ------------------------------------------------------------------------------------------------ linear_dgrad
@dataclass(frozen=True)
class GemmCase:
    id: str
    M: int
    N: int          # reduction length
    K: int          # output width
    mode: int
    dtype: str      # operands
    out: str        # out and aux

    @property
    def engine(self):
        """The engine launches this kernel for fp32 runs only."""
        return self.dtype == "f32"


# (M, N, K): one element; everything below one tile and ragged against the 16-deep step; exactly one tile and one step; one past each;
# several tiles with a ragged last one and 24 steps; the MLP's fc1 dgrad width with 96 steps
GEMM_SHAPES = ((1, 1, 1), (31, 20, 24), (64, 16, 64), (65, 17, 65), (130, 384, 150), (70, 1536, 384))
GEMM_TYPES = (("f32", "f32"), ("bf16", "bf16"), ("bf16", "f32"))
MODE_NAME = {NONE: "none", DGELU: "dgelu", MUL: "mul"}


def gemm_cases():
    return [GemmCase(f"{M}x{N}x{K}-{MODE_NAME[mode]}-{dt}-{o}", M, N, K, mode, dt, o)
            for M, N, K in GEMM_SHAPES for mode in (NONE, DGELU, MUL) for dt, o in GEMM_TYPES]


def gen_gemm(c: GemmCase) -> dict:
    rng = np.random.default_rng(_seed(c.id))
    return dict(dy=to_dt(rng.standard_normal((c.M, c.N), dtype=F), c.dtype), w=to_dt(rng.standard_normal((c.N, c.K), dtype=F) * F(0.5), c.dtype),
                aux=to_dt(rng.standard_normal((c.M, c.K), dtype=F) * F(1.5), c.out))


def gemm_inits(c: GemmCase) -> dict:
    return {"linear_dgrad.out": nan_buf(c.M, c.K, c.out)}


_erf = np.frompyfunc(math.erf, 1, 1)


def erf64(x) -> np.ndarray:
    return _erf(np.asarray(x, np.float64)).astype(np.float64)


def gelu_slope64(x):
    """(gelu_erf'(x), its allowed absolute error on the device) in float64; the module docstring derives the error."""
    x = np.asarray(x, np.float64)
    z, t = x / math.sqrt(2.0), -0.5 * x * x
    erf = erf64(z)
    cdf = 0.5 * (1.0 + erf)
    pdf = np.exp(t) / math.sqrt(2.0 * math.pi)
    q = cdf + x * pdf
    ecdf = 0.5 * (2 * U * np.abs(z) * 2.0 / math.sqrt(math.pi) * np.exp(-z * z) + 2 * U * ERFF_ULP * np.abs(erf)) + U * cdf
    rpdf = 3 * U * np.abs(t) + 2 * U * EXPF_ULP + 2 * U
    return q, SECOND * (ecdf + np.abs(x) * pdf * (rpdf + U) + U * np.abs(q))


def expect_gemm(c: GemmCase, d: dict) -> dict:
    dy, w, aux = widen(d["dy"]).astype(np.float64), widen(d["w"]).astype(np.float64), widen(d["aux"]).astype(np.float64)
    assert np.abs(aux).max() < 8.0
    pre = dy @ w
    e_acc = SECOND * c.N * U * (np.abs(dy) @ np.abs(w))
    if c.mode == NONE:
        ref, bound = pre, e_acc
    else:
        q, eq = gelu_slope64(aux) if c.mode == DGELU else (aux, np.zeros_like(aux))
        ref = pre * q
        bound = SECOND * (e_acc * (np.abs(q) + eq) + np.abs(pre) * eq + U * np.abs(ref))
    if c.out == "bf16":
        bound = bound + UB * (np.abs(ref) + bound)
    return {"linear_dgrad.out": Bounded(ref, bound)}


def _fmaf(a, b, acc):
    """fl32(a b + acc) with the product exact (float64 holds 48 bits) and the sum rounded to 53 bits first: fmaf except where that first
    rounding lands on a fp32 tie -- one fp32 ulp of one term at the most, inside the bound either way."""
    return (a.astype(np.float64) * b.astype(np.float64) + acc.astype(np.float64)).astype(F)


def simulate_gemm(c: GemmCase, d: dict, mutate: str = "") -> dict:
    """mutate: cut_at_16 (the reduction stops at the last multiple of 16) | last_column (the ragged last output column is not
    stored) | aux_transposed (the epilogue reads aux[k][m]; square cases)."""
    dy, w, aux = widen(d["dy"]), widen(d["w"]), widen(d["aux"])
    acc = np.zeros((c.M, c.K), F)
    n_end = c.N // TILE_K * TILE_K if mutate == "cut_at_16" else c.N
    for n in range(n_end):
        acc = _fmaf(dy[:, n:n + 1], w[n:n + 1, :], acc)
    if mutate == "aux_transposed":
        aux = np.ascontiguousarray(aux.T)
    if c.mode == MUL:
        acc = acc * aux
    elif c.mode == DGELU:
        erf = erf64(aux * F(0.70710678118654752440)).astype(F)
        cdf = F(0.5) * (F(1.0) + erf)
        pdf = F(0.39894228040143267794) * np.exp((F(-0.5) * aux * aux).astype(np.float64)).astype(F)
        acc = acc * (cdf + aux * pdf)
    assert acc.dtype == F
    out = gemm_inits(c)["linear_dgrad.out"]
    kk = c.K - 1 if mutate == "last_column" else c.K
    out[:c.M, :kk] = to_dt(acc, c.out)[:, :kk]
    return {"linear_dgrad.out": out}


# ------------------------------------------------------------------------------------------------ completeness
def coverage_gaps() -> list:
    """What the tables must reach and do not; empty for the tables above."""
    gaps = []
    sp = split_cases()
    for c in sp:
        if slices(c.B, c.L, c.D) != c.S:
            gaps.append(f"{c.id}: {slices(c.B, c.L, c.D)} slices, meant to reach {c.S}")
    for w in (True, False):
        for dt in ("f32", "bf16"):
            mine = [c for c in sp if c.with_cls == w and c.dtype == dt]
            geo = [(c, slices(c.B, c.L, c.D), c.L * (c.D // 4)) for c in mine]
            want = {"one thread": lambda c, S, th: th == 1 and c.B == 1, "slices of one image": lambda c, S, th: S == c.B > 1,
                    "a partial last block": lambda c, S, th: th % 256 != 0 and th > 256,
                    "uneven slices at S = 64": lambda c, S, th: S == EMBED_SLICES and c.B % S != 0,
                    "slices of 4 and 5 images (a full group of four and a tail of one)": lambda c, S, th: {b1 - b0 for b0, b1 in slice_bounds(c.B, S)} == {4, 5},
                    "the block limit on slices": lambda c, S, th: S == cdiv(SLICE_BLOCKS, cdiv(th, 256)) < min(c.B, EMBED_SLICES),
                    "a u tail (slice length no multiple of 4)": lambda c, S, th: any((b1 - b0) % 4 for b0, b1 in slice_bounds(c.B, S)),
                    "two strided additions in sum_partials": lambda c, S, th: S > SP_LANES}
            for name, pred in want.items():
                if not any(pred(*g) for g in geo):
                    gaps.append(f"full_grad_split {'cls' if w else 'patch'} {dt}: no case with {name}")
    ze = zero_cases()
    for D in (8, 256, 260, 1024):
        for L in (1, 5):
            if {c.dtype for c in ze if c.D == D and c.L == L} != {"f32", "bf16"}:
                gaps.append(f"zero_token_rows: D {D} L {L} not in both dtypes")
    if not any(c.rows % c.L for c in ze if c.L > 1):
        gaps.append("zero_token_rows: no ragged row count")
    for rpb in (4, 2):
        if not any(zero_rpb(c.D) == rpb and c.rows > ZERO_BLOCKS * rpb for c in ze):
            gaps.append(f"zero_token_rows: no second grid trip at {rpb} rows per block")
    po = pool_cases()
    for D in POOL_DIMS:
        mine = [c for c in po if c.D == D]
        rnd = [c for c in mine if c.kind == "random"]
        if not {1, 2, 3, 4, 5, 8, 9} <= {c.n for c in rnd}:
            gaps.append(f"features_pool D {D}: row counts {sorted({c.n for c in rnd})}")
        if {(c.dtype, c.l2) for c in rnd} != {("f32", False), ("f32", True), ("bf16", False), ("bf16", True)}:
            gaps.append(f"features_pool D {D}: not every branch type and normalisation")
        for name, pred in (("seq = 1", lambda c: c.seq == 1), ("[0, 1) of a longer sequence", lambda c: c.seq > 1 and (c.lo, c.hi) == (0, 1)),
                           ("[1, seq)", lambda c: c.seq > 1 and (c.lo, c.hi) == (1, c.seq)), ("[0, seq)", lambda c: c.seq > 1 and (c.lo, c.hi) == (0, c.seq))):
            if not any(pred(c) for c in rnd):
                gaps.append(f"features_pool D {D}: no {name}")
        if {c.kind for c in mine} != {"random", "const", "zero"}:
            gaps.append(f"features_pool D {D}: exact kinds missing")
    ns = {c.n for c in elem_cases()}
    if not ({1, 255, 257} <= ns and any(n > ELEM_TRIP for n in ns)):
        gaps.append("cast / add_into: sizes")
    if not any(c.rows * (c.D // 4) > ELEM_TRIP and c.rows % c.L for c in pos_cases()):
        gaps.append("add_rows_pos: no second grid trip with a ragged row count")
    ge = gemm_cases()
    for M, N, K in GEMM_SHAPES:
        for mode in (NONE, DGELU, MUL):
            if {(c.dtype, c.out) for c in ge if (c.M, c.N, c.K, c.mode) == (M, N, K, mode)} != set(GEMM_TYPES):
                gaps.append(f"linear_dgrad {M}x{N}x{K} mode {mode}: types")
    for name, pred in (("ragged M", lambda c: c.M % TILE), ("ragged reduction", lambda c: c.N % TILE_K), ("ragged width", lambda c: c.K % TILE),
                       ("exact tiles", lambda c: c.M % TILE == 0 and c.K % TILE == 0 and c.N % TILE_K == 0), ("several tiles each way", lambda c: c.M > TILE and c.K > TILE)):
        if not any(pred(c) for c in ge):
            gaps.append(f"linear_dgrad: no {name}")
    return gaps
