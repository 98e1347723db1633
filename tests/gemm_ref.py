"""Per-element checks of the NT and wgrad GEMMs against fp64, and a Python restatement of their dispatch: the persistent nt3 kernel's
layouts (nt3_route) and the whole chain behind it (fwd_route, wgrad_route).

Torch only (no HIP library): the CPU tests of the checker import it as well as the -m gpu module, which runs the fp64
reference and the comparison on the device (no output of 290 000 rows is copied to the host).

Bounds, per output element, from the exact fp64 value of the same operation (A, W exact bf16, bias fp32):
  pre = A.W^T + b,  s = |A|.|W|^T + |b|,  e_acc = (K / 32 + 2) 2^-24 s       (one fp32 rounding per 32-deep MFMA + the bias add)
  NONE, fp32 out:   |out - pre| <= e_acc + 2^-24 |pre|
  NONE, bf16 out:   |out - pre| <= e_acc + 2^-8 |pre|                         (one bf16 rounding of the fp32 sum)
  MUL:              the same on pre * aux (aux exact bf16; the fp32 product is rounded once more)
  GELU_ACT / GRAD:  the epilogue rounds the fp32 pre-activation to bf16 (c) and applies the fast erf-based GELU (value and
                    slope) to c: an element passes if it lies within one bf16 ulp (+ the documented error of the fast erf) of
                    f(c) for some bf16 value c in [pre - e_acc, pre + e_acc] widened to the bf16 neighbours on either side.

The fallback kernels (everything launch_linear_fwd / launch_linear_wgrad select besides nt3 and the full-M ring) use the same
checks with the rounding count n of their own summation, e_acc = gamma(n) s, gamma(n) = n 2^-24 / (1 - n 2^-24); the count is
read from each kernel's code (rounding_count below says where).  The padded tail of a ragged K adds exact zeros, so n counts
the MFMAs that see a real k, cdiv(K, 32), never the padded length.  Further modes of the fallback kernels:
  RESID (fp32):     out = pre + aux: aux is one more term of the sum (s + |aux|) and adds one rounding.
  GELU:             out is the pre-activation rounded to the output type (checked as NONE); out2 = GELU of the value AS STORED:
                    out2 is compared with f(out) of the kernel's own out, so a GELU of the unrounded sum is a failure.
  DGELU:            out = pre slope(aux), aux exact in the output type; the slope's own error eq enters as |pre| eq.
  fp32 outputs of GELU_GRAD / GELU_ACT: c is the fp32 sum itself, anywhere in [pre - e_acc, pre + e_acc]; both functions are
                    Lipschitz (|gelu'| <= 1.13, |gelu''| <= 0.8), so |out - f(pre)| <= L e_acc + the function's own error.
Which GELU a kernel evaluates is read from its code: the MFMA kernels gelu_fast_pair (Abramowitz-Stegun, ERF_ABS / CDF_ABS
above), gemm_generic_kernel gelu_erf / gelu_erf_grad (erff, __expf).  Where no bf16 rounding of the argument follows (fp32 outputs,
GELU's out2, DGELU's factor) CDF_ABS, which allows four fp32 half-ulps around the formula's own 1.5e-7, is too small for the
fp32 evaluation itself: v_rcp_f32's ulp reaches the result through P'(t) (about 3.4 at t = 1) and the Horner steps add theirs, 3e-7
on the device at |x| = 0.08.  fast_budget counts that evaluation operation by operation; the nt3 table keeps CDF_ABS behind its
one-ulp interval.  The error budget of the latter is the one of
tests/engine_kernels_ref.py (gelu_slope64 there): ERFF_ULP = 4 and EXPF_ULP = 2 are ALLOWED, NOT MEASURED (ROCm's accuracy
table is not among the files of an installation); the formula is restated here in torch and the constants are imported.
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, replace
from pathlib import Path

import torch

NONE, GELU_GRAD, MUL, GELU_ACT, KEEP = 0, 4, 5, 6, 77   # epilogue modes of mae_linear_fwd; 77 = NONE with ordinary stores (nt3 only)
GELU, RESID, DGELU = 1, 2, 3                            # the epilogues nt3 declines (mae_hip.h MAE_EPI_*)
MODE_NAME = {NONE: "none", KEEP: "77", GELU_GRAD: "gelu_grad", MUL: "mul", GELU_ACT: "gelu_act", GELU: "gelu", RESID: "resid", DGELU: "dgelu"}
ALL_MODES = (NONE, GELU, RESID, DGELU, GELU_GRAD, MUL, GELU_ACT)
U32 = 2.0 ** -24          # fp32 unit roundoff
U16 = 2.0 ** -8           # bf16 unit roundoff
ERF_ABS = 1.5e-7          # |error| of the Abramowitz-Stegun 7.1.26 erf that gelu_fast_pair evaluates
CDF_ABS = ERF_ABS / 2 + 4 * U32 / 2   # its cumulative distribution (erf / 2) after the fp32 operations around it

# ------------------------------------------------------------------------------------------------ bf16 ordering
def _bf16_key(x: torch.Tensor) -> torch.Tensor:
    """Monotone integer key of bf16 values (consecutive keys = neighbouring bf16 values; +0 and -0 share 0)."""
    b = x.view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def _key_to_double(k: torch.Tensor) -> torch.Tensor:
    b = torch.where(k >= 0, k, (-k) | 0x8000)
    b = torch.where(b >= 0x8000, b - 0x10000, b)
    return b.to(torch.int16).view(torch.bfloat16).double()


def _bracket(x: torch.Tensor, up: bool) -> torch.Tensor:
    """Key of the largest bf16 <= x (up = False) or the smallest bf16 >= x (up = True), x in fp64."""
    k = _bf16_key(x.float().bfloat16())
    c = _key_to_double(k)
    return torch.where(c < x, k + 1, k) if up else torch.where(c > x, k - 1, k)


def bf16_ulp(y: torch.Tensor) -> torch.Tensor:
    """Spacing of the bf16 values at |y| (fp64)."""
    _, e = torch.frexp(y)
    return torch.ldexp(torch.ones_like(y), (e.to(torch.int32) - 8).clamp_min(-133))


def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def gelu_slope64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def gamma(n) -> float:
    """Relative error of a sum with at most n fp32 roundings along any path (Higham's gamma_n)."""
    return n * U32 / (1 - n * U32)


def erf_budget(x):
    """(ecdf, eq): allowed absolute error of the device's 0.5 (1 + erff(x / sqrt 2)) and of gelu_erf_grad(x), fp64 tensors.
    The derivation and the constants are those of tests/engine_kernels_ref.py (module docstring there, gelu_slope64):
    ERFF_ULP and EXPF_ULP are allowed, not measured."""
    from tests.engine_kernels_ref import ERFF_ULP, EXPF_ULP
    from tests.ln_ref import SECOND
    z, t = x / math.sqrt(2.0), -0.5 * x * x
    erf = torch.erf(z)
    cdf = 0.5 * (1.0 + erf)
    pdf = torch.exp(t) / math.sqrt(2.0 * math.pi)
    q = cdf + x * pdf
    ecdf = 0.5 * (2 * U32 * z.abs() * 2.0 / math.sqrt(math.pi) * torch.exp(-z * z) + 2 * U32 * ERFF_ULP * erf.abs()) + U32 * cdf
    rpdf = 3 * U32 * t.abs() + 2 * U32 * EXPF_ULP + 2 * U32
    return ecdf, SECOND * (ecdf + x.abs() * pdf * (rpdf + U32) + U32 * q.abs())


AS_COEF = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)   # Abramowitz-Stegun 7.1.26, a1 .. a5
RCP_ULP, EXP2_ULP = 1, 1   # v_rcp_f32 / v_exp_f32 as the ISA manual states them (1 ulp = 2 u); taken from there, not measured


def fast_budget(x):
    """(ecdf, eslope): absolute error of gelu_fast_pair's cdf and slope as fp32 evaluates them (common.cuh), fp64 tensors.  The
    formula's own error is ERF_ABS / 2; the rest is counted operation by operation:
      t = rcp(fma(|x|, c0, 1)): the constant and the fma round (2 u), v_rcp_f32 RCP_ULP: et = 2 u + 2 u RCP_ULP, relative
      P = t (a1 + t (a2 + ..)): four fmas and a product, each u |its result|, carried to the end by factors t <= 1: u sum |h_k|;
          the error of t moves P by |P'(t)| t et
      e = exp2(fl(fl(x x) c)): the argument is off by 3 u |arg|, i.e. e by 1.5 u x^2, v_exp_f32 EXP2_ULP: re = 1.5 u x^2 + 2 u EXP2_ULP
      h = fma(fl(P e), -0.5, 0.5): (e eP + P e (re + u)) / 2 + u |h|;  cdf = copysign(h, x) + 0.5 rounds once more
      slope = fma(fl(x c1), e, cdf): |x| pdf (re + 2 u) + ecdf + u |slope|"""
    from tests.ln_ref import SECOND
    ax = x.abs()
    t = 1.0 / (1.0 + 0.3275911 / math.sqrt(2.0) * ax)
    e = torch.exp(-0.5 * x * x)
    a1, a2, a3, a4, a5 = AS_COEF
    et = 2 * U32 + 2 * U32 * RCP_ULP
    h, hsum = a5 * t + a4, 0
    for a in (a3, a2, a1):
        hsum = hsum + h.abs()
        h = h * t + a
    P = h * t
    hsum = hsum + h.abs() + P.abs()
    dP = (a1 + t * (2 * a2 + t * (3 * a3 + t * (4 * a4 + t * 5 * a5)))).abs()
    eP = U32 * hsum + dP * t * et
    re = 1.5 * U32 * x * x + 2 * U32 * EXP2_ULP
    half = 0.5 * torch.erf(ax / math.sqrt(2.0))
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))
    ecdf = ERF_ABS / 2 + 0.5 * (e * eP + P * e * (re + U32)) + U32 * half + U32 * cdf
    pdf = e / math.sqrt(2.0 * math.pi)
    eslope = ax * pdf * (re + 2 * U32) + ecdf + U32 * (cdf + x * pdf).abs()
    return SECOND * ecdf, SECOND * eslope


def gelu_errors(kind: str):
    """(value error, slope error) as functions of the fp64 argument c, absolute, before the output rounding.
    fast: gelu_fast_pair (common.cuh) where a bf16 rounding follows (the nt3 table's GELU_ACT / GELU_GRAD): the error of its cdf
    times |c| and the x exp(-x^2 / 2) / sqrt(2 pi) (<= 0.25) term to a few fp32 ulps; fast32: the same function counted operation
    by operation (fast_budget), for fp32 outputs and for GELU / DGELU, where no candidate interval absorbs it;
    erf: gelu_erf = fl(fl(0.5 c) fl(1 + erff(..))): |c| ecdf and the product's rounding, gelu_erf_grad: eq (erf_budget)."""
    if kind == "fast":   # (the users add 2 u |f| for the last fp32 operations)
        return (lambda c: CDF_ABS * c.abs()), (lambda c: CDF_ABS + 0.25 * 8 * U32 + 0 * c)
    if kind == "fast32":
        return (lambda c: c.abs() * fast_budget(c)[0] + U32 * gelu64(c).abs()), (lambda c: fast_budget(c)[1])
    assert kind == "erf", kind
    return (lambda c: c.abs() * erf_budget(c)[0] + U32 * gelu64(c).abs()), (lambda c: erf_budget(c)[1])


LIP_GELU, LIP_SLOPE = 1.13, 0.8     # max |gelu'| (1.129 at x = 1.41) and max |gelu''| (2 pdf(0) = 0.798), rounded up


# ------------------------------------------------------------------------------------------------ report
@dataclass
class Report:
    what: str
    tile: tuple = (1, 1)
    n: int = 0
    bad: int = 0
    nan: int = 0
    fill: int = 0
    worst_ratio: float = 0.0          # max error / bound over the finite elements
    worst: tuple = ()                 # (row, col, got, ref, bound) of that element
    first_bad: tuple = ()             # (row, col) of the first failing element (NaN / fill included)

    @property
    def ok(self) -> bool:
        return self.n > 0 and self.bad == 0 and self.nan == 0 and self.fill == 0

    def merge(self, r: "Report") -> None:
        self.n += r.n; self.bad += r.bad; self.nan += r.nan; self.fill += r.fill
        if r.worst and (not self.worst or r.worst_ratio > self.worst_ratio):
            self.worst_ratio, self.worst = r.worst_ratio, r.worst
        if r.first_bad and not self.first_bad:
            self.first_bad = r.first_bad

    def __str__(self) -> str:
        bm, bn = self.tile
        s = f"{self.what}: {self.bad} of {self.n} outside the bound, {self.nan} NaN, {self.fill} at the fill value; worst error/bound {self.worst_ratio:.3g}"
        if self.worst:
            r, c, got, ref, bd = self.worst
            s += f" at (row {r}, col {c}, tile {r // bm},{c // bn}): got {got:.9g}, fp64 {ref:.9g}, bound {bd:.3g}"
        if self.first_bad:
            r, c = self.first_bad
            s += f"; first failing element (row {r}, col {c}, tile {r // bm},{c // bn})"
        return s


def _tally(rep: Report, r0: int, got: torch.Tensor, ref: torch.Tensor, dist: torch.Tensor, bound: torch.Tensor, fill) -> None:
    """got / ref / dist / bound: (rows, N) fp64 tensors of one row chunk starting at row r0."""
    n_cols = got.shape[1]
    nan = torch.isnan(got)
    at_fill = torch.zeros_like(nan) if fill is None or (isinstance(fill, float) and math.isnan(fill)) else (got == fill)
    ratio = torch.where(nan, torch.zeros_like(dist), dist / bound)
    bad = (ratio > 1) | torch.isnan(ratio) | torch.isinf(ratio)
    r = Report(rep.what, rep.tile, n=got.numel(), bad=int(bad.sum()), nan=int(nan.sum()), fill=int(at_fill.sum()))
    i = int(torch.nan_to_num(ratio, nan=float("inf")).flatten().argmax())
    r.worst_ratio = float(ratio.flatten()[i])
    r.worst = (r0 + i // n_cols, i % n_cols, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i]))
    anyfail = bad | nan | at_fill
    if bool(anyfail.any()):
        j = int(anyfail.flatten().to(torch.int32).argmax())
        r.first_bad = (r0 + j // n_cols, j % n_cols)
    rep.merge(r)


def check_nt(A, W, bias, aux, mode, out, out2=None, *, tile=(256, 192), fill=float("nan"), chunk_elems=1 << 24, what="nt",
             roundings=None, gelu="fast") -> Report:
    """out[M, N] (and out2 for GELU_GRAD: out = slope, out2 = value; for GELU: out = pre-activation, out2 = value) of
    mae_linear_fwd(A[M, K], W[N, K], bias, mode, aux) against fp64, element by element (module docstring).  Runs where the
    tensors live.  roundings: the fp32 roundings of the kernel's sum along any path (rounding_count; None = K / 32 + 2, the nt3
    count at K % 64 == 0); gelu: "fast" (gelu_fast_pair, the MFMA kernels) or "erf" (gelu_erf, gemm_generic_kernel)."""
    M, K = A.shape
    N = W.shape[0]
    f32 = out.dtype == torch.float32
    Wd = W.double()
    Wa = Wd.abs()
    b = bias.double() if bias is not None else None
    e_k = (K / 32 + 2) * U32 if roundings is None else gamma(roundings)
    e_k1 = (K / 32 + 3) * U32 if roundings is None else gamma(roundings + 1)
    val_err, slope_err = gelu_errors(gelu)                                     # behind a candidate interval of bf16 pre-activations
    val_err1, slope_err1 = gelu_errors("fast32" if gelu == "fast" else gelu)   # at one known argument
    rep = Report(what, tile)
    rows = max(1, chunk_elems // max(N, 1))
    for r0 in range(0, M, rows):
        r1 = min(M, r0 + rows)
        a = A[r0:r1].double()
        pre = a @ Wd.t()
        s = a.abs() @ Wa.t()
        if b is not None:
            pre += b
            s += b.abs()
        if mode == RESID:   # the fp32 residual is one more term, its addition one more rounding
            q = aux[r0:r1].double()
            pre, e = pre + q, e_k1 * (s + q.abs())
        else:
            e = e_k * s
        del a, s
        if mode in (NONE, KEEP, MUL, RESID, GELU, DGELU):
            u = U32 if f32 else U16
            if mode == MUL:
                q = aux[r0:r1].double()
                ref, e = pre * q, e * q.abs()
                u = u + U32
            elif mode == DGELU:
                x = aux[r0:r1].double()
                q, eq = gelu_slope64(x), slope_err1(x) + 2 * U32 * gelu_slope64(x).abs()
                ref, e = pre * q, e * (q.abs() + eq) + pre.abs() * eq
                u = u + U32
            else:
                ref = pre
            got = out[r0:r1].double()
            _tally(rep, r0, got, ref, (got - ref).abs(), e * (1 + u) + u * ref.abs() + 1e-40, fill)
            if mode == GELU:   # the activation of the value as stored: no interval, the kernel's own out is the argument
                fc = gelu64(got)
                d = val_err1(got) + 2 * U32 * fc.abs()
                got2 = out2[r0:r1].double()
                _tally(rep, r0, got2, fc, (got2 - fc).abs(), d + u * (fc.abs() + d) + 1e-40, fill)
            continue
        if f32:   # GELU_GRAD / GELU_ACT with fp32 outputs: c is the fp32 sum, f is Lipschitz
            targets = [(out, gelu_slope64, slope_err1, LIP_SLOPE)] if mode == GELU_GRAD else []
            targets.append((out2 if mode == GELU_GRAD else out, gelu64, val_err1, LIP_GELU))
            for o, f, d_abs, lip in targets:
                got, ref = o[r0:r1].double(), f(pre)
                bound = (lip * e + d_abs(pre)) * (1 + 2.0 ** -16) + 3 * U32 * ref.abs() + 1e-40
                _tally(rep, r0, got, ref, (got - ref).abs(), bound, fill)
            continue
        # GELU epilogues: the bf16 pre-activations c the kernel may have seen (lo .. hi), f(c) for each; near zero, where the
        # interval holds more than five bf16 values, anything between f(lo) and f(hi) (both functions are monotone there)
        lo, hi = _bracket(pre - e, up=False), _bracket(pre + e, up=True)
        wide = (hi - lo) > 4
        del pre, e
        # absolute error of the fast slope: its cdf plus x exp(-x^2 / 2) / sqrt(2 pi) (<= 0.25) to a few fp32 ulps
        targets = [(out, gelu_slope64, slope_err)] if mode == GELU_GRAD else []
        targets.append((out2 if mode == GELU_GRAD else out, gelu64, val_err))
        for o, f, d_abs in targets:
            got = o[r0:r1].double()
            best = torch.full_like(got, float("inf"))
            best_f = torch.zeros_like(got)
            best_t = torch.ones_like(got)
            for j in range(5):
                k = lo + j
                c = _key_to_double(torch.minimum(k, hi))
                fc = f(c)
                tol = bf16_ulp(fc) + d_abs(c) + 2 * U32 * fc.abs()
                r = torch.where(k <= hi, (got - fc).abs() / tol, torch.full_like(got, float("inf")))
                take = r < best
                best, best_f, best_t = torch.where(take, r, best), torch.where(take, fc, best_f), torch.where(take, tol, best_t)
            if bool(wide.any()):
                clo, chi = _key_to_double(lo), _key_to_double(hi)
                flo, fhi = f(clo), f(chi)
                fmin, fmax = torch.minimum(flo, fhi), torch.maximum(flo, fhi)
                tol = bf16_ulp(fmax.abs().maximum(fmin.abs())) + d_abs(clo.abs().maximum(chi.abs())) + 2 * U32 * fmax.abs().maximum(fmin.abs())
                r = torch.maximum(fmin - got, got - fmax).clamp_min(0) / tol
                take = wide & (r < best)
                best, best_f, best_t = torch.where(take, r, best), torch.where(take, got.clamp(fmin, fmax), best_f), torch.where(take, tol, best_t)
            best = torch.where(torch.isnan(got), torch.full_like(got, float("inf")), best)
            _tally(rep, r0, got, best_f, best * best_t, best_t, fill)
    return rep


def check_wgrad(dY, A, dW, db=None, *, fill=float("nan"), chunk_elems=1 << 24, what="wgrad", roundings=None, db_roundings=None, tile=(192, 192)):
    """dW[N, K] = dY[M, N]^T A[M, K] and db = column sums of dY (fp32 outputs) against fp64; e_acc over the M-long reduction.
    roundings / db_roundings: the fp32 roundings along any path of the kernel's sum (rounding_count; None = M / 32 + 2, the ring
    kernels' MFMAs); the bound holds for any order of the additions, so also for atomics."""
    M, N = dY.shape
    K = A.shape[1]
    Ad = A.double()
    Aa = Ad.abs()
    e_m = (M / 32 + 2) * U32 if roundings is None else gamma(roundings)
    e_b = e_m if db_roundings is None else gamma(db_roundings)
    rep = Report(what, tile)
    cols = max(1, chunk_elems // max(M, 1))
    for n0 in range(0, N, cols):
        n1 = min(N, n0 + cols)
        y = dY[:, n0:n1].double()
        ref = y.t() @ Ad
        s = y.abs().t() @ Aa
        got = dW[n0:n1].double()
        _tally(rep, n0, got, ref, (got - ref).abs(), e_m * s + U32 * ref.abs() + 1e-40, fill)
    if db is None:
        return rep, None
    y = dY.double()
    ref, s = y.sum(0), y.abs().sum(0)
    repb = Report(what + " db", (1, tile[0]))
    got = db.double()[None]
    _tally(repb, 0, got, ref[None], (got - ref[None]).abs(), (e_b * s + U32 * ref.abs() + 1e-40)[None], fill)
    return rep, repb


# ------------------------------------------------------------------------------------------------ NT dispatch
LAYOUTS = {  # (NI, MI, WM) of launch_nt3 -> name; w2 = two 4-wave workgroups per CU (MAE_GEMM_NT=v3w2)
    (8, 3, 4): "<8,3,4>", (12, 2, 8): "<12,2,8>", (6, 3, 4): "<6,3,4>", (6, 4, 4): "<6,4,4>", (4, 4, 4): "<4,4,4>",
    (6, 4, 2): "<6,4,2>", (4, 4, 2): "<4,4,2>",
}
W2_LAYOUTS = {(6, 4, 2), (4, 4, 2)}


def geo(layout):
    NI, MI, WM = layout
    WN = 1 if WM == 8 else 2
    return 16 * MI * WM, 16 * NI * WN, WN * WM      # BM, BN, waves


@dataclass(frozen=True)
class Route:
    layout: tuple
    mode: int
    f32: bool
    bias: bool
    bm: int
    bn: int
    tiles: int
    tiles_n: int
    grid: int
    per_wg: int       # most tiles one persistent workgroup owns
    dr: int           # column step of a workgroup's next tile (G mod tiles_n)
    a_nt: int

    @property
    def label(self):
        return (LAYOUTS[self.layout], MODE_NAME[self.mode], "f32" if self.f32 else "bf16", self.bias)


def _cdiv(a, b):
    return -(-a // b)


@dataclass(frozen=True)
class Knobs:
    """The dispatcher's A/B switches: MAE_GEMM_NT=v3w2 (read per call), MAE_NT_BM / MAE_NT_WN1 / MAE_NT_N256 / MAE_NT_KEEP /
    MAE_NT3_ANT (read once per process)."""
    w2: bool = False
    bm: int = 0
    wn1: int = 1
    n256: int = 1
    keep: int = 64 << 20
    ant_max: int = 1

    @staticmethod
    def from_env(env=None) -> "Knobs":
        env = os.environ if env is None else env
        v = env.get("MAE_GEMM_NT")
        return Knobs(w2=(v == "v3w2"), bm=int(env.get("MAE_NT_BM", 0)), wn1=int(env.get("MAE_NT_WN1", 1)),
                     n256=int(env.get("MAE_NT_N256", 1)), keep=int(env.get("MAE_NT_KEEP", 64 << 20)), ant_max=int(env.get("MAE_NT3_ANT", 1)))


def nt3_route(M, N, K, mode, f32, bias, num_cus, knobs: Knobs = Knobs()):
    """k_gemm_nt3.hip mfma_linear_fwd_v3 -> launch_nt3_ni -> launch_nt3, restated: the layout, epilogue mode, tiles and
    persistent grid of one bf16 mae_linear_fwd call, or None when the call goes to another kernel."""
    if K % 64 or K < 192 or (N % 128 and N % 192) or M < 1:
        return None
    if (M + 512) * K * 2 >= 1 << 32 or N * K * 2 >= 1 << 32 or (M + 512) * N * (4 if f32 else 2) >= 1 << 32:
        return None
    if mode == NONE:
        if not f32 and knobs.keep > 0 and M * N * 2 <= knobs.keep and N % 256:
            mode = KEEP
    elif mode in (GELU_GRAD, GELU_ACT, MUL):
        if f32:
            return None
    else:
        return None

    def prefer_bm192():
        if knobs.bm == 192:
            return True
        if knobs.bm == 256:
            return False
        t256, t192 = _cdiv(M, 256) * (N // 192), _cdiv(M, 192) * (N // 192)
        return _cdiv(t192, num_cus) * 192 * 100 < _cdiv(t256, num_cus) * 256 * 85

    if knobs.n256 and N % 256 == 0 and not knobs.w2:
        lay = (8, 3, 4)
    elif N % 192 == 0:
        if knobs.w2:
            lay = (6, 4, 2)
        elif prefer_bm192():
            lay = (6, 3, 4)
        elif knobs.wn1 and not f32:
            lay = (12, 2, 8)
        else:
            lay = (6, 4, 4)
    else:
        lay = (4, 4, 2) if knobs.w2 else (4, 4, 4)
    bm, bn, waves = geo(lay)
    tiles_n = N // bn
    tiles = _cdiv(M, bm) * tiles_n
    grid = min(tiles, num_cus * (1 if waves == 8 else 2))
    return Route(lay, mode, f32, bool(bias), bm, bn, tiles, tiles_n, grid, _cdiv(tiles, grid), grid % tiles_n, int(tiles_n <= knobs.ant_max))


def reachable_labels(num_cus, knobs: Knobs = Knobs()):
    """Every (layout, mode, output dtype, bias) the dispatcher selects for some shape under `knobs`."""
    out = set()
    for M in (1, 100, 5000, 20000, 65536, 72000, 290000, 1000000):
        for N in (128, 192, 256, 384, 576, 640, 768, 1152, 1536):
            for mode in (NONE, GELU_GRAD, MUL, GELU_ACT):
                for f32 in (False, True):
                    for bias in (False, True):
                        r = nt3_route(M, N, 384, mode, f32, bias, num_cus, knobs)
                        if r is not None:
                            out.add(r.label)
    return out


# ------------------------------------------------------------------------------------------------ the engine's launches
@dataclass(frozen=True)
class Net:
    name: str
    D: int          # encoder width
    Dd: int         # decoder / predictor width
    P: int          # patch pixels (patch embed K)
    PO: int         # prediction width
    Me: int
    Md: int
    Mp: int
    mlp: int = 4
    fwd_only_encoder: bool = False   # I-JEPA target encoder: GELU_ACT instead of GELU_GRAD


def _plan(B, L, k):
    """engine.hip make_plan: Me = B k, Md = B L, Mp = B (L - k)."""
    return B * k, B * L, B * (L - k)


NETS = [
    Net("vits8", 384, 192, 192, 192, *_plan(2000, 145, 36)),                 # ViT-S/8 96 px MAE, B = 2000 (the bench workload)
    Net("vits8_dec512", 384, 512, 192, 192, *_plan(2000, 145, 36)),          # the same encoder, 512-wide decoder
    Net("vitb16", 768, 512, 768, 768, *_plan(512, 197, 49)),                # ViT-B/16 224 px MAE, B = 512 (dec512 decoder)
    # ViT-L/14 I-JEPA, B = 256: the target encoder over all 256 patches (forward only) and a context pass with a sampled
    # draw of 100 context tokens and 4 target blocks of 44 tokens (make_jepa_plan: Me = B k, Md = 4 B (k + m), Mp = 4 B m)
    Net("vitl14_target", 1024, 384, 588, 1024, 256 * 256, 1, 1, fwd_only_encoder=True),
    Net("vitl14_ctx", 1024, 384, 588, 1024, 256 * 100, 4 * 256 * 144, 4 * 256 * 44),
]


def engine_launches(net: Net, part=("enc", "dec", "misc")):
    """(name, M, N, K, mode, f32 out, bias) of the NT GEMMs one bf16 pretrain step issues (engine.hip linear() / dgrad())."""
    D, Dd, h = net.D, net.Dd, net.mlp
    out = []
    if "misc" in part:
        out.append(("patch embed", net.Me, D, net.P, NONE, True, True))
    for stack, M, d in (("enc", net.Me, D), ("dec", net.Md, Dd)):
        if stack not in part or (stack == "dec" and net.fwd_only_encoder):
            continue
        fwd_only = stack == "enc" and net.fwd_only_encoder
        out += [(f"{stack} qkv", M, 3 * d, d, NONE, False, True), (f"{stack} proj", M, d, d, NONE, False, True),
                (f"{stack} fc1", M, h * d, d, GELU_ACT if fwd_only else GELU_GRAD, False, True),
                (f"{stack} fc2", M, d, h * d, NONE, False, True)]
        if not fwd_only:
            out += [(f"{stack} fc2 dgrad", M, h * d, d, MUL, False, False), (f"{stack} fc1 dgrad", M, d, h * d, NONE, False, False),
                    (f"{stack} proj dgrad", M, d, d, NONE, False, False), (f"{stack} qkv dgrad", M, d, 3 * d, NONE, False, False)]
    if "misc" in part and not net.fwd_only_encoder:
        out += [("dec embed", net.Me, Dd, D, NONE, False, True), ("pred head", net.Mp, net.PO, Dd, NONE, True, True),
                ("pred dgrad", net.Mp, Dd, net.PO, NONE, False, False), ("dec embed dgrad", net.Me, D, Dd, NONE, False, False)]
    return [(f"{net.name} {n}",) + tuple(rest) for n, *rest in out]


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    mode: int
    f32: bool
    bias: bool
    w2: bool = False

    @property
    def id(self):
        return f"{self.name.replace(' ', '_')}-{self.M}x{self.N}x{self.K}-{MODE_NAME[self.mode]}-{'f32' if self.f32 else 'bf16'}-{'b' if self.bias else 'nb'}{'-w2' if self.w2 else ''}"

    def route(self, num_cus, knobs: Knobs = Knobs()):
        return nt3_route(self.M, self.N, self.K, self.mode, self.f32, self.bias, num_cus, replace(knobs, w2=self.w2 or knobs.w2))


def _edge_cases(num_cus):
    c = []
    # persistent grids with exactly num_cus tiles and one fewer / one more (one round, one idle CU, one workgroup with 2 tiles):
    # 256-row tiles on N = 192, 192-row tiles on N = 256 / 512 (one tile column, ragged last tile for the +1 cases)
    c += [Case("tiles = cus-1", 256 * (num_cus - 1), 192, 384, NONE, False, True), Case("tiles = cus", 256 * num_cus, 192, 384, NONE, False, True),
          Case("tiles = cus+1", 192 * (num_cus + 1) - 37, 256, 384, NONE, False, True),
          Case("tiles = cus, 192x256", 192 * (num_cus // 2), 512, 256, GELU_GRAD, False, True),
          Case("tiles = cus+1, 192x256", 192 * (num_cus + 1) - 5, 256, 256, MUL, False, False)]
    # a workgroup's next tile in another column (G mod tiles_n != 0), several tiles per workgroup, for every production layout
    c += [Case("dr, 12x2x8", 72000, 576, 384, GELU_ACT, False, True), Case("dr, 6x4x4 f32", 72000, 576, 192, NONE, True, True),
          Case("dr, 6x4x4 f32 nb", 150000, 1152, 192, NONE, True, False), Case("dr, 8x3x4", 40000, 768 + 768, 256, NONE, True, False),
          Case("dr, 4x4x4", 60001, 640, 192, NONE, False, True), Case("dr, 6x3x4", 45000, 576, 192, NONE, False, True)]
    # M below one tile, M = 1
    c += [Case("M < tile", 100, 384, 384, NONE, False, True), Case("M = 1", 1, 192, 192, GELU_GRAD, False, True),
          Case("M = 1 f32", 1, 192, 384, NONE, True, False), Case("M = 1, 256", 1, 256, 192, MUL, False, False),
          Case("M = 1, 128", 1, 128, 256, NONE, False, True)]
    # one tile column (tiles_n = 1: non-temporal activation stream) for N = 128, 192, 256; ragged for 192 and 256 rows
    c += [Case("a_nt N=128", 50001, 128, 256, GELU_GRAD, False, True), Case("a_nt N=192", 100001, 192, 576, NONE, False, False),
          Case("a_nt N=256", 40001, 256, 512, GELU_ACT, False, True), Case("a_nt N=128 f32", 20001, 128, 192, NONE, True, True)]
    # the remaining (layout, mode, output dtype, bias) combinations of the default dispatch, several tiles per workgroup
    c += [Case("12x2x8 none nb", 400000, 192, 192, NONE, False, False), Case("12x2x8 384 nb", 100000, 384, 192, NONE, False, False),
          Case("12x2x8 gelu_grad nb", 72000, 576, 192, GELU_GRAD, False, False), Case("12x2x8 gelu_act nb", 72000, 576, 192, GELU_ACT, False, False),
          Case("12x2x8 mul b", 72000, 576, 192, MUL, False, True), Case("12x2x8 mul nb", 72000, 576, 384, MUL, False, False),
          Case("12x2x8 gelu_grad b", 72000, 1152, 192, GELU_GRAD, False, True), Case("12x2x8 77 b", 25000, 1152, 192, NONE, False, True),
          Case("6x3x4 77 nb", 5000, 576, 192, NONE, False, False), Case("6x3x4 none b", 130000, 1152, 192, NONE, False, True),
          Case("6x3x4 f32 b", 5000, 384, 192, NONE, True, True), Case("6x3x4 f32 nb", 5000, 384, 192, NONE, True, False),
          Case("6x3x4 gelu_grad nb", 5000, 1152, 192, GELU_GRAD, False, False), Case("6x3x4 gelu_act", 5000, 1152, 192, GELU_ACT, False, True),
          Case("6x3x4 gelu_act nb", 5000, 576, 192, GELU_ACT, False, False), Case("6x3x4 mul b", 5000, 576, 192, MUL, False, True),
          Case("6x3x4 mul nb", 5000, 1152, 192, MUL, False, False), Case("6x3x4 77 b", 5000, 1152, 384, NONE, False, True),
          Case("6x3x4 gelu_grad b", 5000, 576, 192, GELU_GRAD, False, True), Case("6x3x4 none nb", 130000, 1152, 192, NONE, False, False),
          Case("8x3x4 none b", 70000, 1536, 192, NONE, False, True), Case("8x3x4 none nb", 70000, 512, 192, NONE, False, False),
          Case("8x3x4 f32 b", 30000, 512, 256, NONE, True, True), Case("8x3x4 gelu_grad nb", 30000, 512, 256, GELU_GRAD, False, False),
          Case("8x3x4 gelu_act nb", 30000, 768, 256, GELU_ACT, False, False), Case("8x3x4 mul b", 30000, 512, 256, MUL, False, True),
          Case("4x4x4 none nb", 120000, 640, 192, NONE, False, False), Case("4x4x4 77 nb", 30000, 640, 192, NONE, False, False),
          Case("4x4x4 f32 nb", 30000, 640, 192, NONE, True, False), Case("4x4x4 gelu_grad nb", 30000, 640, 192, GELU_GRAD, False, False),
          Case("4x4x4 gelu_act", 30000, 640, 192, GELU_ACT, False, True), Case("4x4x4 gelu_act nb", 30000, 640, 192, GELU_ACT, False, False),
          Case("4x4x4 mul", 30000, 640, 192, MUL, False, True), Case("4x4x4 mul nb", 30000, 896, 192, MUL, False, False)]
    return c


def _w2_cases():
    """The two 4-wave layouts (MAE_GEMM_NT=v3w2, read per call): every mode, output dtype and bias."""
    c = []
    for N, K in ((576, 192), (640, 256)):
        for mode, f32, M in ((NONE, False, 120000), (NONE, False, 20000), (NONE, True, 20001), (GELU_GRAD, False, 20001),
                             (MUL, False, 20000), (GELU_ACT, False, 20001)):
            for bias in (False, True):
                c.append(Case("w2", M, N, K, mode, f32, bias, w2=True))
    return c


def nt_cases(num_cus):
    """The -m gpu table: every NT launch of the four configurations (deduplicated), the edges and the remaining combinations."""
    seen, out = set(), []
    for net in TABLE_NETS:
        for name, M, N, K, mode, f32, bias in engine_launches(net):
            key = (M, N, K, mode, f32, bias)
            if key in seen or nt3_route(M, N, K, mode, f32, bias, num_cus) is None:
                continue
            seen.add(key)
            out.append(Case(name, M, N, K, mode, f32, bias))
    return out + _edge_cases(num_cus) + _w2_cases()


def coverage(cases, num_cus, knobs: Knobs = Knobs()):
    """label -> [(case, route)] of the cases that reach nt3."""
    cov = {}
    for c in cases:
        r = c.route(num_cus, knobs)
        if r is not None:
            cov.setdefault(r.label, []).append((c, r))
    return cov


def coverage_gaps(cases, num_cus):
    """What the table misses: (layout, mode, dtype, bias) labels the dispatcher can select (default knobs, and v3w2) that no
    case reaches, and production layouts / modes never compared at a shape with several tiles per workgroup."""
    cov = coverage(cases, num_cus)
    want = reachable_labels(num_cus) | reachable_labels(num_cus, replace(Knobs(), w2=True))
    gaps = sorted(str(x) for x in want - set(cov))
    must_multi = [("<12,2,8>", "none", "bf16"), ("<12,2,8>", "77", "bf16"), ("<6,4,4>", "none", "f32"), ("<8,3,4>", "none", "bf16"),
                  ("<6,3,4>", "77", "bf16"), ("<4,4,4>", "none", "bf16")]
    for lay, mode, dt in must_multi:
        if not any(lbl[:3] == (lay, mode, dt) and r.per_wg >= 2 for lbl, v in cov.items() for _, r in v):
            gaps.append(f"{lay} {mode} {dt}: no case with several tiles per workgroup")
    for lay in ("<12,2,8>", "<6,4,4>", "<8,3,4>", "<4,4,4>"):
        if not any(lbl[0] == lay and r.per_wg >= 2 and r.dr != 0 for lbl, v in cov.items() for _, r in v):
            gaps.append(f"{lay}: no case whose workgroups change column between tiles")
    tiles = {r.tiles for v in cov.values() for _, r in v}
    for t in (num_cus - 1, num_cus, num_cus + 1):
        if t not in tiles:
            gaps.append(f"no case with exactly {t} tiles")
    for N in (128, 192, 256):
        if not any(r.tiles_n == 1 and r.a_nt and c.N == N for v in cov.values() for c, r in v):
            gaps.append(f"no one-column case for N = {N}")
    if not any(c.M == 1 for v in cov.values() for c, _ in v):
        gaps.append("no M = 1 case")
    for bm in (192, 256):
        if not any(r.bm == bm and c.M % 192 and c.M % 256 and r.per_wg >= 2 for v in cov.values() for c, r in v):
            gaps.append(f"no ragged last tile row on {bm}-row tiles")
    return gaps


# ------------------------------------------------------------------------------------------------ wgrad shapes
WGRAD_M = {"vits8 dec": 290000, "vits8 enc": 72000, "dec512": 100864, "vitl14": 65536}


def wgrad_pairs():
    """(name, M, (N0, K0), (N1, K1)) of the engine's wgrad_pair launches: a block's fc2 + fc1 and proj + qkv."""
    out = []
    for name, M, d in (("vits8 dec", 290000, 192), ("vits8 enc", 72000, 384), ("dec512", 100864, 512), ("vitl14", 65536, 1024)):
        out += [(f"{name} fc2+fc1", M, (d, 4 * d), (4 * d, d)), (f"{name} proj+qkv", M, (d, d), (3 * d, d))]
    return out


def wgrad_singles():
    """(name, M, N, K) of the engine's single wgrad launches (patch / decoder embed / prediction head) and one ragged M-split tail."""
    return [("vits8 patch", 72000, 384, 192), ("vits8 dec embed", 72000, 192, 384), ("vits8 pred", 218000, 192, 192),
            ("vitb16 pred", 512 * 148, 768, 512), ("vitl14 qkv", 65536, 3072, 1024), ("dec512 fc2", 100864, 512, 2048),
            ("ragged split tail", 290000 + 77, 192, 768), ("ragged split tail 2", 72000 + 5, 1536, 384)]


# ------------------------------------------------------------------------------------------------ ISA scan
_FUNC = re.compile(r"^(_Z\S*gemm_nt3_kernel\S*):")
_STORE = re.compile(r"^\s*(buffer_store_dword\w*)\s+(.*)$")


def scan_nt3_stores(asm: str):
    """{kernel symbol: [(line number, instruction) of every buffer_store_dword* whose soffset is not the literal 0]} and
    {kernel symbol: number of buffer stores}."""
    cur, bad, count = None, {}, {}
    for no, line in enumerate(asm.splitlines(), 1):
        m = _FUNC.match(line)
        if m:
            cur = m.group(1); bad.setdefault(cur, []); count.setdefault(cur, 0)
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None:
            continue
        s = _STORE.match(line)
        if s:
            count[cur] += 1
            ops = [o.strip() for o in s.group(2).split(";")[0].split(",")]
            soff = ops[3].split()[0] if len(ops) > 3 else ""
            if soff != "0":
                bad[cur].append((no, line.strip()))
    return bad, count


def makefile_cxxflags(makefile: Path):
    m = re.search(r"^CXXFLAGS\s*\?=\s*(.*)$", makefile.read_text(), re.M)
    return m.group(1).split()


# ------------------------------------------------------------------------------------------------ the whole dispatch
# Restated from the C++ (ssrl_vit_mae_jepa_amd/csrc): launch_linear_fwd and nt_sel (k_gemm.hip, the chain v3 -> v2 -> v1 -> generic and
# the whole-string MAE_GEMM_NT match), mfma_linear_fwd_v2 / launch_nt2_ni (k_gemm_nt2.hip, shape test and tile choice), prefer_bm192
# (k_gemm.hip), mfma_linear_fwd / launch_nt_ni (k_gemm_nt1.hip, shape and 16-byte alignment test, NI), launch_generic (k_gemm.hip, the
# operand type x output type x split-K pick of the generic kernel), launch_linear_wgrad (k_gemm.hip, the `M <= 4096 ? M : 2048`
# split-K rule and the colsum grid), epi_values8 (gemm_dev.cuh, the fast-GELU value step of the nt1 and nt2 epilogues; EpiDev in
# k_gemm.hip is the generic kernel's exact-erf one), mfma_linear_wgrad, wgrad_splits, ring_shape_ok, ring_splits and
# env_sel (k_gemm_tn.hip, `m_chunk = round_up(cdiv(M, S), 64)`, the instantiation switch and the whole-string MAE_WGRAD match).
@dataclass(frozen=True)
class KRoute:
    label: str
    tile: tuple = (64, 64)     # rows x columns of one output tile (reports name the tile of a failing element)
    roundings: int = 0         # fp32 roundings along any path of one output element's sum (rounding_count)
    gelu: str = "fast"         # which GELU the epilogue evaluates
    ordered: bool = True       # the additions of an element happen in a fixed order: two launches give the same bits
    layout: tuple = ()         # nt2: (NI, MI)
    S: int = 1                 # M-splits of the MFMA weight gradients
    m_chunk: int = 0
    nz: int = 1                # split-K chunks of the generic weight gradient
    colsum: bool = False       # the bias gradient comes from colsum_kernel + sum_partials_kernel
    db_roundings: int = 0


def _round_up(a, b):
    return _cdiv(a, b) * b


def rounding_count(label: str, K: int, S: int = 1, m_chunk: int = 0, nz: int = 1) -> int:
    """fp32 roundings along any path of one output element's sum, per kernel, K = the reduction length:
    nt1 / nt2 / nt3   one v_mfma_f32_16x16x32_bf16 per 32 k; the MFMAs of the zero-filled tail add exact zeros, so cdiv(K, 32)
                      of them round (gemm_nt_kernel's `for ks < 2` inside `for kt < nk`), + 1 allowed for the MFMA's own sum of
                      its 32 products (not specified bit for bit) + 1 for the bias add in the epilogue: cdiv(K, 32) + 2.
    generic           gemm_generic_kernel: `acc[i][j] = fmaf(a[i], b[j], acc[i][j])` K times in ascending k (zero-filled tail
                      terms are exact), + the bias add of EpiDev::apply + 1: K + 2.
    tn / ring         per split cdiv(rows, 32) MFMAs over rows = m_chunk (M when S = 1) + 1 for the MFMA's own sum; with S > 1
                      slab_reduce_kernel: slice sl adds slabs sl, sl + 8, ..: cdiv(S, 8) additions, then `t += red[k]` 7 times.
    generic_tn        chunk = `M <= 4096 ? M : 2048` sequential fmafs per split-K chunk; generic_tn_splitk adds the nz partial
                      sums into the zeroed dW with atomicAdd in no fixed order: nz more roundings whatever the order."""
    if label.startswith("nt"):
        return _cdiv(K, 32) + 2
    if label.startswith("generic<"):
        return K + 2
    if label.startswith("tn<") or label == "ring":
        rows = K if S == 1 else min(m_chunk, K)
        return _cdiv(rows, 32) + 1 + (_cdiv(S, 8) + 7 if S > 1 else 0)
    assert label.startswith("generic_tn"), label
    return (K if K <= 4096 else 2048) + (nz if nz > 1 else 0)


NT_SEL = {"v1": (1, False), "v2": (2, False), "v3": (3, False), "v3w2": (3, True)}   # kNtSel; anything else is v3


def fwd_route(M, N, K, dt, mode, f32_out, aligned=True, sel="v3", *, num_cus=256) -> KRoute:
    """The kernel instantiation that serves mae_linear_fwd(M, N, K) with operands dt ("bf16" | "f32"), epilogue `mode`, output type,
    every pointer 16-byte aligned or not, under MAE_GEMM_NT = sel.  check_epi's rules (RESID writes fp32, fp32 operands write fp32)
    are the caller's."""
    assert mode in ALL_MODES and (mode != RESID or f32_out) and (dt == "bf16" or f32_out)
    if dt != "bf16":
        return KRoute("generic<f32,f32>", (64, 64), rounding_count("generic<", K), "erf")
    first, w2 = NT_SEL.get(sel, NT_SEL["v3"])
    if first == 3 and aligned:
        r3 = nt3_route(M, N, K, mode, f32_out, True, num_cus, Knobs(w2=w2))
        if r3 is not None:
            return KRoute("nt3", (r3.bm, r3.bn), rounding_count("nt3", K), layout=r3.layout)
    if first >= 2 and aligned and K % 64 == 0 and K >= 192 and (N % 128 == 0 or N % 192 == 0):
        if N % 192 == 0:   # launch_nt2_ni: 192-row tiles whenever they save a round (prefer_bm192 with a 95 % margin)
            t256, t192 = _cdiv(M, 256) * (N // 192), _cdiv(M, 192) * (N // 192)
            lay = (6, 3) if _cdiv(t192, num_cus) * 192 * 100 < _cdiv(t256, num_cus) * 256 * 95 else (6, 4)
        else:
            lay = (4, 4)
        return KRoute("nt2", (64 * lay[1], 32 * lay[0]), rounding_count("nt2", K), layout=lay)
    if aligned and K % 8 == 0 and N % 8 == 0 and K >= 32 and N >= 16:
        if K % 64 or N % 64:
            return KRoute("nt1<2,RG>", (128, 64), rounding_count("nt1", K))
        if N % 128 == 0:
            return KRoute("nt1<NI=4>", (128, 128), rounding_count("nt1", K))
        return KRoute("nt1<NI=2>", (128, 64), rounding_count("nt1", K))
    return KRoute("generic<bf16,f32>" if f32_out else "generic<bf16,bf16>", (64, 64), rounding_count("generic<", K), "erf")


def wgrad_splits(M, N, K):
    tn = 128 if N % 128 == 0 or N % 64 else 64
    tk = 128 if K % 128 == 0 or K % 64 else 64
    tiles = _cdiv(N, tn) * _cdiv(K, tk)
    S = max(1, 512 // tiles)
    S = min(S, max(1, M // 512))
    return min(S, 64)


def ring_shape_ok(M, N, K):
    if M < 4096:
        return False
    if N % 192 == 0 and K % 192 == 0:
        return True
    if N % 8 or K % 8 or N < 192 or K < 192:
        return False
    return N * K * 100 >= _cdiv(N, 192) * _cdiv(K, 192) * 192 * 192 * 75


def ring_splits(M, tiles, nk_sum, s_min, num_cus):
    smax = min(512, max(1, M // 256))
    t1 = M / 64 * 1.5
    slab = nk_sum * 8.0 / 5.0e6
    best, best_cost = s_min, 1e30
    for S in range(s_min, smax + 1):
        cost = _cdiv(tiles * S, num_cus) * t1 / S + S * slab
        if cost < best_cost * 0.999:
            best_cost, best = cost, S
    return best


def wgrad_route(M, N, K, dt, has_db, has_scratch=True, sel=None, *, num_cus=256) -> KRoute:
    """The kernel instantiation that serves mae_linear_wgrad(M, N, K) (16-byte aligned pointers) under MAE_WGRAD = sel
    (v1 | v3r | v4 | v4b; anything else, None included, leaves the default)."""
    assert not has_db or (has_scratch and N % 4 == 0)
    if dt == "bf16" and N % 8 == 0 and K % 8 == 0 and N >= 16 and K >= 16:
        ring = sel != "v1" and ring_shape_ok(M, N, K)
        S = ring_splits(M, _cdiv(N, 192) * _cdiv(K, 192), N * K, 1, num_cus) if ring else wgrad_splits(M, N, K)
        if S == 1 or has_scratch:
            m_chunk = _round_up(_cdiv(M, S), 64)
            if ring:
                label, tile = "ring", (192, 192)
            elif N % 64 or K % 64:
                label, tile = "tn<4,4,RG>", (128, 128)
            else:
                ni, ki = (4 if N % 128 == 0 else 2), (4 if K % 128 == 0 else 2)
                label, tile = f"tn<{ni},{ki}>", (32 * ni, 32 * ki)
            n = rounding_count(label, M, S, m_chunk)
            return KRoute(label, tile, n, S=S, m_chunk=m_chunk, db_roundings=n)
    chunk = M if M <= 4096 else 2048
    nz = _cdiv(M, chunk)
    G = min(_cdiv(M, 4), 256)     # colsum_kernel: each wave adds every (4 G)-th row, 3 additions join the 4 waves, sum_partials_kernel
    dbn = _cdiv(M, 4 * G) + 3 + G  # adds the G partials in a fixed order (+ G is an upper bound: its longest path is cdiv(G, 32) + min(G, 32))
    label = "generic_tn" if nz == 1 else "generic_tn_splitk"
    return KRoute(label, (64, 64), rounding_count(label, M, nz=nz), ordered=nz == 1, nz=nz, colsum=bool(has_db), db_roundings=dbn)


# ------------------------------------------------------------------------------------------------ what nt_cases leaves out
# configs/mae.yaml, the reference's shipped default: 96 px, patch 8 (P = PO = 192), encoder width 144, decoder width 192, B = 2000.
# Its decoder launches have the ViT-S/8 widths, which the nt3 table covers; its encoder launches all leave nt3 (table = False keeps
# nt_cases as it was).
MAE_YAML = Net("mae_yaml", 144, 192, 192, 192, *_plan(2000, 145, 36))
NETS.append(MAE_YAML)
TABLE_NETS = [n for n in NETS if n is not MAE_YAML]


def dropped_engine_launches(num_cus=256):
    """The engine_launches rows of every net that nt_cases skips because nt3 declines them (deduplicated as there)."""
    seen, out = set(), []
    for net in NETS:
        for row in engine_launches(net):
            if row[1:] not in seen and nt3_route(*row[1:], num_cus) is None:
                seen.add(row[1:])
                out.append(row)
    return out


# ------------------------------------------------------------------------------------------------ the fallback table
@dataclass(frozen=True)
class FwdCase:
    name: str
    M: int
    N: int
    K: int
    mode: int = NONE
    f32: bool = False
    bias: bool = True
    dt: str = "bf16"
    sel: str = None            # MAE_GEMM_NT for this call
    misalign: bool = False     # the bias pointer one float off 16-byte alignment

    def route(self, num_cus=256):
        return fwd_route(self.M, self.N, self.K, self.dt, self.mode, self.f32, not self.misalign, self.sel or "v3", num_cus=num_cus)

    @property
    def id(self):
        return (f"{self.route().label}-{self.M}x{self.N}x{self.K}-{MODE_NAME[self.mode]}-{self.dt}-{'f32' if self.f32 else 'bf16'}-"
                f"{'b' if self.bias else 'nb'}{'-' + self.sel if self.sel else ''}{'-misaligned' if self.misalign else ''}")

    @property
    def key(self):
        return (self.route().label, MODE_NAME[self.mode], "f32" if self.f32 else "bf16", self.bias)


@dataclass(frozen=True)
class WgradCase:
    name: str
    M: int
    N: int
    K: int
    db: bool = True
    dt: str = "bf16"
    sel: str = None            # MAE_WGRAD for this call
    pair: tuple = ()           # (N1, K1): mae_linear_wgrad_pair with this second problem

    def route(self, num_cus=256):
        return wgrad_route(self.M, self.N, self.K, self.dt, self.db, True, self.sel, num_cus=num_cus)

    @property
    def id(self):
        r = self.route()
        extra = f"-S{r.S}" if r.S > 1 else (f"-nz{r.nz}" if r.nz > 1 else "")
        return (f"{r.label}{extra}-{self.M}x{self.N}x{self.K}-{self.dt}-{'db' if self.db else 'nodb'}{'-' + self.sel if self.sel else ''}"
                f"{'-pair%dx%d' % self.pair if self.pair else ''}")

    @property
    def key(self):
        return (self.route().label, self.dt, self.db)


def _mode_cross(name, M, N, K, dt="bf16", outs=(False, True), biases=(True, False), modes=ALL_MODES):
    return [FwdCase(name, M, N, K, mode, f32, bias, dt) for mode in modes for f32 in outs for bias in biases if mode != RESID or f32]


RG_SHAPES = [(1, 16, 32),        # the minimum of every dimension, one K step
             (70, 24, 40),       # N < tile width, K < one step
             (129, 144, 144),    # two row tiles with a clamped last one; N = 2 64 + 16; K = 2 64 + 16
             (130, 432, 144), (100, 576, 144), (257, 144, 576),   # the width-144 encoder's qkv, fc1 and fc2
             (127, 64, 72),      # full columns, ragged K only
             (300, 200, 64),     # full K; the last tile column holds one 8-column group
             (128, 72, 200)]
NI2_SHAPES = [(200, 192, 128), (129, 320, 64), (513, 64, 128)]
NI4_SHAPES = [(129, 128, 64), (300, 256, 128), (1, 384, 128)]
V1_SHAPES = [(300, 384, 384),    # six K steps through both LDS buffers
             (300, 192, 256),
             (1100, 192, 128)]   # 27 tiles, not a multiple of the 8 XCDs for xcd_remap
NT2_SHAPES = [(1, 128, 192), (300, 192, 192), (700, 384, 256)]
NT2_F32_SHAPES = [(300, 192, 192), (300, 128, 256)]
NT2_BM256 = (24600, 384, 256)    # gemm_nt2_kernel<.., 6, 4>: launch_nt2_ni takes 256-row tiles on N % 192 == 0 only when 192-row ones
                                 # need a second round of the CUs (24 577 .. 32 768 rows on 256 CUs); 96 full tiles and a ragged one
DROPPED_M = 130                  # the row count the dropped engine launches are repeated at: two 128-row tiles, a ragged last one


def fallback_fwd_cases(num_cus=256):
    c = []
    # nt1: every epilogue x output type x bias on one shape per instantiation, NONE on the other shapes
    for lbl, shapes, full in (("nt1<2,RG>", RG_SHAPES, (129, 144, 144)), ("nt1<NI=2>", NI2_SHAPES, (200, 192, 128)), ("nt1<NI=4>", NI4_SHAPES, (300, 256, 128))):
        for M, N, K in shapes:
            c += _mode_cross(lbl, M, N, K) if (M, N, K) == full else [FwdCase(lbl, M, N, K, NONE, M % 2 == 0, True)]
    c += [FwdCase("nt1<NI=4>" if N % 128 == 0 else "nt1<NI=2>", M, N, K, NONE, False, True, sel="v1") for M, N, K in V1_SHAPES]
    # nt2: the epilogues nt3 declines
    for M, N, K in NT2_SHAPES:
        c += _mode_cross("nt2", M, N, K, biases=(True, False) if M == 300 else (True,), modes=(GELU, RESID, DGELU))
    for M, N, K in NT2_F32_SHAPES:
        c += _mode_cross("nt2", M, N, K, outs=(True,), biases=(True, False) if N == 192 else (True,), modes=(GELU_GRAD, GELU_ACT, MUL))
    c.append(FwdCase("nt2", *NT2_BM256, GELU, False, True))
    # generic, bf16 operands
    # the ViT-L/14 patch embed (K % 8 == 4); K < 32; N % 8 != 0; an nt1 shape whose bias pointer is one float off 16-byte alignment
    c += [FwdCase("generic<bf16,f32>", 70, 1024, 588, NONE, True, True), FwdCase("generic<bf16,bf16>", 31, 20, 24, NONE, False, True),
          FwdCase("generic<bf16,bf16>", 37, 12, 64, NONE, False, True), FwdCase("generic<bf16,bf16>", 70, 144, 144, NONE, False, True, misalign=True)]
    c += [replace(x, name="generic<bf16,f32>" if x.f32 else "generic<bf16,bf16>") for x in _mode_cross("", 65, 68, 24)]
    # generic, fp32 operands: partial tiles in all three dimensions and K not a multiple of the 16-deep step; the width-144 encoder
    c += _mode_cross("generic<f32,f32>", 65, 68, 17, "f32", outs=(True,))
    c += _mode_cross("generic<f32,f32>", 130, 144, 192, "f32", outs=(True,), biases=(True,))
    # every engine launch nt_cases drops, at a small M with its own (N, K, mode, output type, bias)
    have = {(x.N, x.K, x.mode, x.f32, x.bias) for x in c if not x.misalign and x.sel is None and x.dt == "bf16"}
    for name, M, N, K, mode, f32, bias in dropped_engine_launches(num_cus):
        if (N, K, mode, f32, bias) not in have:
            have.add((N, K, mode, f32, bias))
            c.append(FwdCase("generic<bf16,f32>" if K % 8 else "nt1<2,RG>", DROPPED_M, N, K, mode, f32, bias))   # test_gemm_checker pins these two
    return c


TN_SHAPES = {"tn<4,4>": [(128, 128)], "tn<4,2>": [(128, 64), (256, 192)], "tn<2,4>": [(64, 128), (192, 256)], "tn<2,2>": [(64, 64), (192, 192)],
             "tn<4,4,RG>": [(144, 144), (432, 144), (144, 576), (24, 16), (200, 72)]}
TN_M = (1, 63, 64, 65, 700, 1100)   # below / at / above one 64-row step, S = 1 with a ragged step, S = 2 with a ragged second chunk
EMPTY_CHUNKS = [(8200, 128, 128),   # S = 16, m_chunk = 576: chunk 15 starts at row 8640 > M and must contribute exact zeros
                (33000, 64, 64)]    # S = 64, m_chunk = 576: six empty chunks


def fallback_wgrad_cases():
    c = []
    for label, shapes in TN_SHAPES.items():
        for i, (N, K) in enumerate(shapes):
            for M in (TN_M if i == 0 else (65, 1100)):
                c.append(WgradCase(label, M, N, K))
            if i == 0:
                c += [WgradCase(label, 65, N, K, db=False), WgradCase(label, 1100, N, K, db=False)]
    c.append(WgradCase("tn<4,4,RG>", 3000, 144, 144))                        # S = 5
    c += [WgradCase("tn<4,4>" if N == 128 else "tn<2,2>", M, N, K) for M, N, K in EMPTY_CHUNKS]
    # a ring-capable shape pinned to gemm_tn_kernel, and on the ring (16 splits of 320 rows on 256 CUs: the last three are empty there too)
    c += [WgradCase("tn<2,2>", 4100, 192, 192, sel="v1"), WgradCase("ring", 4100, 192, 192), WgradCase("ring", 4100, 192, 192, db=False)]
    c.append(WgradCase("tn<4,4,RG>", 5000, 144, 144, pair=(432, 144)))        # below M = 8192: two single launches sharing one scratch
    # K % 8 != 0 (the ViT-L/14 patch embed's widths) or fp32 operands
    c += [WgradCase("generic_tn", 130, 1024, 588), WgradCase("generic_tn", 100, 144, 192, dt="f32"), WgradCase("generic_tn", 70, 20, 24, dt="f32"),
          WgradCase("generic_tn", 70, 20, 24, dt="f32", db=False), WgradCase("generic_tn", 70, 20, 20, db=False)]
    # nz = 3 with a last chunk of one row; the patch embed's K
    c += [WgradCase("generic_tn_splitk", 4097, 24, 20, dt="f32"), WgradCase("generic_tn_splitk", 4100, 72, 588),
          WgradCase("generic_tn_splitk", 4097, 24, 20, dt="f32", db=False), WgradCase("generic_tn_splitk", 4100, 72, 588, db=False)]
    # colsum_kernel: a second column block holding one float4 group (N = 260), waves without a row (M = 3), the grid capped at 256
    # blocks with strided rows (M = 1025), both operand types
    c += [WgradCase("generic_tn", 3, 260, 24, dt="f32"), WgradCase("generic_tn", 1025, 260, 20, dt="f32"), WgradCase("generic_tn", 1025, 260, 20)]
    return c


def exact_forward(A, W, bias, aux, mode, f32):
    """On small integers every partial sum is exact in fp32, so NONE / RESID / MUL outputs and GELU's stored pre-activation are
    determined bit for bit: the fp64 result (fp32 outputs) or its single round-to-nearest-even (bf16 outputs).  None for the
    epilogues that evaluate a GELU on `out`."""
    if mode not in (NONE, RESID, MUL, GELU):
        return None
    pre = A.double() @ W.double().t()
    if bias is not None:
        pre = pre + bias.double()
    if mode == RESID:
        pre = pre + aux.double()
    if mode == MUL:
        pre = pre * aux.double()
    assert float(pre.abs().max()) < 2 ** 24
    return pre if f32 else pre.float().bfloat16().double()


def guard_intact(buf, rows) -> bool:
    """The NaN-filled rows behind row `rows` - 1 of an output buffer are untouched."""
    return bool(torch.isnan(buf[rows:]).all())


FWD_LABELS = ("nt1<NI=4>", "nt1<NI=2>", "nt1<2,RG>", "nt2", "generic<bf16,bf16>", "generic<bf16,f32>", "generic<f32,f32>")
WGRAD_LABELS = ("ring", "tn<4,4>", "tn<4,2>", "tn<2,4>", "tn<2,2>", "tn<4,4,RG>", "generic_tn", "generic_tn_splitk")


def fallback_reachable():
    """Every (label, mode, output type, bias) the forward dispatch can select outside nt3 with the default MAE_GEMM_NT, and every
    (label, operand type, db) of the weight gradients."""
    fwd = set()
    for M, N, K in ((100, 256, 128), (100, 192, 128), (100, 144, 144), (100, 192, 192), (100, 128, 256), (100, 68, 24)):
        for dt in ("bf16", "f32"):
            for mode in ALL_MODES:
                for f32 in (False, True):
                    if (mode == RESID or dt == "f32") and not f32:
                        continue
                    lbl = fwd_route(M, N, K, dt, mode, f32).label
                    if lbl != "nt3":
                        fwd |= {(lbl, MODE_NAME[mode], "f32" if f32 else "bf16", b) for b in (False, True)}
    wg = set()
    for M, N, K in ((700, 128, 128), (700, 128, 64), (700, 64, 128), (700, 64, 64), (700, 144, 144), (5000, 192, 192), (700, 20, 24), (5000, 20, 24)):
        for dt in ("bf16", "f32"):
            for db in (False, True):
                wg.add((wgrad_route(M, N, K, dt, db).label, dt, db))
    return fwd, wg


def fallback_coverage_gaps(cases, num_cus=256):
    """What the fallback table (forward and weight-gradient cases together) misses: reachable (label, mode, output type, bias) and
    (label, operand type, db) that no case reaches, and the edges the kernels can get wrong."""
    fw = [c for c in cases if isinstance(c, FwdCase)]
    wg = [c for c in cases if isinstance(c, WgradCase)]
    want_f, want_w = fallback_reachable()
    gaps = sorted(str(x) for x in want_f - {c.key for c in fw}) + sorted(str(x) for x in want_w - {c.key for c in wg})
    fr = [(c, c.route(num_cus)) for c in fw]
    wr = [(c, c.route(num_cus)) for c in wg]

    def need(ok, what):
        if not ok:
            gaps.append(what)

    for lbl in ("nt1<NI=4>", "nt1<2,RG>", "nt2"):
        need(any(r.label == lbl and c.M == 1 for c, r in fr), f"{lbl}: no M = 1 case")
    for lbl in ("nt1<NI=4>", "nt1<NI=2>", "nt1<2,RG>"):
        need(any(r.label == lbl and c.M > 128 and c.M % 128 for c, r in fr), f"{lbl}: no second row tile with a clamped last one")
    rg = [c for c, r in fr if r.label == "nt1<2,RG>"]
    need(any(c.K < 64 for c in rg), "nt1<2,RG>: no K below one step")
    need(any(c.K % 64 and c.K > 64 and c.N % 64 == 0 for c in rg), "nt1<2,RG>: no ragged K with full columns")
    need(any(c.K % 64 == 0 and c.N % 64 == 8 for c in rg), "nt1<2,RG>: no last tile column of one 8-column group with full K")
    need(any(c.N < 64 for c in rg), "nt1<2,RG>: no N below the tile width")
    v1 = [c for c, r in fr if c.sel == "v1" and r.label.startswith("nt1")]
    need(any(c.K >= 384 for c in v1), "nt1 under MAE_GEMM_NT=v1: no case with six K steps")
    need(any((_cdiv(c.M, r.tile[0]) * (c.N // r.tile[1])) % 8 for c, r in fr if c.sel == "v1"), "nt1 under MAE_GEMM_NT=v1: no tile count off a multiple of 8")
    for bm in (192, 256):
        need(any(r.label == "nt2" and r.tile[0] == bm and bm < c.M < 2 * bm for c, r in fr), f"nt2: no two row tiles with a ragged last one at {bm}-row tiles")
    need({r.layout for c, r in fr if r.label == "nt2"} >= {(6, 3), (4, 4)} | ({(6, 4)} if num_cus == 256 else set()), "nt2: a tile layout is never reached")
    gen = [c for c, r in fr if r.label.startswith("generic<bf16")]
    need(any(c.K < 32 for c in gen), "generic: no K < 32")
    need(any(c.N % 8 for c in gen), "generic: no N % 8 != 0")
    need(any(c.K % 8 == 4 and c.K > 64 for c in gen), "generic: no K % 8 == 4 (the ViT-L/14 patch embed)")
    need(any(c.misalign for c in gen), "generic: no misaligned pointer on an nt1 shape")
    need(any(c.dt == "f32" and c.K % 16 and c.M % 64 and c.N % 64 for c in fw), "generic<f32,f32>: no partial tiles in all three dimensions")
    for lbl in TN_SHAPES:
        ms = {c.M for c, r in wr if r.label == lbl}
        need(ms >= set(TN_M), f"{lbl}: M values missing {sorted(set(TN_M) - ms)}")
        need(any(r.label == lbl and r.S == 2 and c.M % r.m_chunk % 64 for c, r in wr), f"{lbl}: no S = 2 with a ragged second chunk")
    need(any(r.S > 2 and r.label == "tn<4,4,RG>" for c, r in wr), "tn<4,4,RG>: no case with more than two splits")
    need(sum(1 for c, r in wr if r.label.startswith("tn<") and (r.S - 1) * r.m_chunk >= c.M) >= 2, "tn: fewer than two cases whose last chunks are empty")
    need(any(c.sel == "v1" and ring_shape_ok(c.M, c.N, c.K) for c in wg), "tn: no ring-capable shape under MAE_WGRAD=v1")
    need(any(c.pair and c.M < 8192 for c in wg), "no mae_linear_wgrad_pair case below M = 8192")
    need(any(r.label == "generic_tn_splitk" and c.M % 2048 == 1 for c, r in wr), "generic_tn_splitk: no last chunk of one row")
    for dt in ("bf16", "f32"):
        need(any(r.colsum and c.dt == dt and c.N == 260 for c, r in wr), f"colsum {dt}: no N = 260")
    need(any(r.colsum and c.M < 4 for c, r in wr), "colsum: no M < 4")
    need(any(r.colsum and c.M > 1024 and c.M % 4 for c, r in wr), "colsum: no M beyond the 256-block grid")
    unordered = {r.label for _, r in fr + wr if not r.ordered}
    need(unordered <= {"generic_tn_splitk"}, f"unordered routes besides generic_tn_splitk: {sorted(unordered)}")
    return gaps
