"""Per-element checks of the NT and wgrad GEMMs against fp64, and a Python restatement of the NT kernel's dispatch.

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
"""
from __future__ import annotations

import math
import os
import re
from dataclasses import dataclass, replace
from pathlib import Path

import torch

NONE, GELU_GRAD, MUL, GELU_ACT, KEEP = 0, 4, 5, 6, 77   # epilogue modes of mae_linear_fwd; 77 = NONE with ordinary stores (nt3 only)
MODE_NAME = {NONE: "none", KEEP: "77", GELU_GRAD: "gelu_grad", MUL: "mul", GELU_ACT: "gelu_act"}
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


def check_nt(A, W, bias, aux, mode, out, out2=None, *, tile=(256, 192), fill=float("nan"), chunk_elems=1 << 24, what="nt") -> Report:
    """out[M, N] (and out2 for GELU_GRAD: out = slope, out2 = value) of mae_linear_fwd(A[M, K], W[N, K], bias, mode, aux)
    against fp64, element by element (module docstring).  Runs where the tensors live."""
    M, K = A.shape
    N = W.shape[0]
    f32 = out.dtype == torch.float32
    Wd = W.double()
    Wa = Wd.abs()
    b = bias.double() if bias is not None else None
    e_k = (K / 32 + 2) * U32
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
        e = e_k * s
        del a, s
        if mode in (NONE, KEEP, MUL):
            u = U32 if f32 else U16
            if mode == MUL:
                q = aux[r0:r1].double()
                ref, e = pre * q, e * q.abs()
                u = u + U32
            else:
                ref = pre
            got = out[r0:r1].double()
            _tally(rep, r0, got, ref, (got - ref).abs(), e * (1 + u) + u * ref.abs() + 1e-40, fill)
            continue
        # GELU epilogues: the bf16 pre-activations c the kernel may have seen (lo .. hi), f(c) for each; near zero, where the
        # interval holds more than five bf16 values, anything between f(lo) and f(hi) (both functions are monotone there)
        lo, hi = _bracket(pre - e, up=False), _bracket(pre + e, up=True)
        wide = (hi - lo) > 4
        del pre, e
        # absolute error of the fast slope: its cdf plus x exp(-x^2 / 2) / sqrt(2 pi) (<= 0.25) to a few fp32 ulps
        targets = [(out, gelu_slope64, lambda c: CDF_ABS + 0.25 * 8 * U32)] if mode == GELU_GRAD else []
        targets.append((out2 if mode == GELU_GRAD else out, gelu64, lambda c: CDF_ABS * c.abs()))
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


def check_wgrad(dY, A, dW, db=None, *, fill=float("nan"), chunk_elems=1 << 24, what="wgrad"):
    """dW[N, K] = dY[M, N]^T A[M, K] and db = column sums of dY (fp32 outputs) against fp64; e_acc over the M-long reduction."""
    M, N = dY.shape
    K = A.shape[1]
    Ad = A.double()
    Aa = Ad.abs()
    e_m = (M / 32 + 2) * U32
    rep = Report(what, (192, 192))
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
    repb = Report(what + " db", (1, 192))
    got = db.double()[None]
    _tally(repb, 0, got, ref[None], (got - ref[None]).abs(), (e_m * s + U32 * ref.abs() + 1e-40)[None], fill)
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
    for net in NETS:
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
