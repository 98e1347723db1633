"""Per-element checks of the attention kernels (k_attention_mfma.hip, k_attention.hip) against fp64: the reference, the bounds,
a Python restatement of the dispatch, the case table, the input families and a torch fp32 emulation of the MFMA arithmetic.

Torch only (no HIP library): tests/test_attn_ref_host.py runs it on the CPU, tests/test_gpu_attention.py where the tensors live.

Layout: qkv (B, T, 3 H hd) = [q | k | v] x [head] x [hd] per token row, out / d_out (B, T, H hd), lse (B, H, T), d_qkv like qkv.
Inside this module every per-head quantity is (B, H, T, hd) or (B, H, T, T) [query t, key j] in fp64.

Reference (from the operand values as stored, scale = hd^-1/2 in fp64):
  S = scale Q K^T, P = softmax(S), O = P V, lse = logsumexp(S), M = max_j S
  dP = dO V^T, D = sum_j P dP, dS = P (dP - D), dV = P^T dO, dQ = scale dS K, dK = scale dS^T Q
The backward is judged alone: it is given lse = fp32(reference lse) and out = activation-type(reference O).

Notation of the bounds: u32 = 2^-24, u16 = 2^-8 (unit roundoffs to nearest), A_tj = scale sum_d |q_td k_jd|.
E_EXP, E_LOG: relative error of v_exp_f32 / v_log_f32 (and of the __expf / __logf built on them).  The ROCm tree ships no
document that states an ulp figure for them (nothing under its doc or include directories names one), so both start from 1 ulp of
the fp32 result, 2^-23 = 2 u32 relative.  Not tuned.

MFMA path (bf16), constants counted from k_attention_mfma.hip:
  c_acc(K) = K / 32 + 1     an fp32 accumulation of exact bf16 products through K / 32 MFMA steps: one rounding per step and one
                            for the alignment of the partial sums inside a step
  eS_tj  = c_acc(HD) u32 A_tj + 5 u32 |S_tj| + 6 u32 |M_t|   (forward; nats)
             scale = 1 / sqrtf(hd) (2 roundings), kLog2e (1), sl2 = scale * kLog2e (1): 4 u32 |S|; the same 4 and the rounding of
             mn2 = m * sl2 on |M|; the rounding of fmaf(s, sl2, -mn2) is u32 |S - M| <= u32 (|S| + |M|)
  out    : bracket of  O -+ e,  e = (u16 + 2 max_j eS_tj + E_EXP + c u32) sum_j P_tj |v_jd|
             u16: P is rounded to bf16 once (pack8) while lsum adds the unrounded values; 2 max eS: numerator and denominator;
             c = (8 nch + 2) [lsum: 8 adds per chunk per lane, 2 across the lane groups] + 2 [E_EXP of the terms of lsum]
                 + c_acc(32 nch) [P V] + 2 [inv = 1 / lsum, oacc * inv] + 3 nch if online [oacc *= alpha, lsum * alpha + ps]
  online : alpha = exp2(m sl2 - mn2) multiplies oacc and lsum alike, but not the chunk that follows: its error re-weights the earlier
             keys against the later ones in numerator and denominator.  Each of the nch rescales carries E_EXP and the roundings of
             m sl2, mn2 and their difference, 3 u32 max_j |S_tj| nats: eS_tj gains nch (E_EXP + 3 u32 max_j |S_tj|) in the online form.
  lse    : max_j eS_tj + 4 u32 |M_t| + u32 |log lsum| + (8 nch + 2) u32 + E_EXP + E_LOG' (+ 2 nch u32 online: lsum * alpha + ps)
             4 u32 |M|: m * scale (scale 2, product 1) and the final add; E_LOG' = (E_LOG + 2 u32) |log lsum| (v_log_f32, times
             ln 2 rounded, product rounded)
  eP_tj  = c_acc(HD) u32 A_tj + 5 u32 |S_tj| + 4 u32 |lse_t| log2e + E_EXP      (backward, relative, recomputed P)
             lse given to fp32 (1), li = lse * kLog2e (constant 1, product 1), the fmaf's rounding on the lse side (1)
  ddP_tj = c_acc(HD) u32 sum_d |dO_td v_jd|
  dD_t   = (u16 + c u32) sum_d |dO_td O_td|, c = 8 + log2(HD / 8) + 1      chunk-loop form: 8 fmaf per lane, shuffle adds, fp32 O is
                                                                            exact in bf16 only to u16 (the rounded `out`)
         = sum_j P_tj (eP_tj |dP_tj| + ddP_tj) + (8 nch + 2) u32 sum_j P_tj |dP_tj|      DPM form (never reads O)
  ddS_tj = u16 |dS_tj| + P_tj (eP_tj |dP_tj - D_t| + ddP_tj + dD_t) + 2 u32 |dS_tj|      (the subtraction and the product)
  dQ     : bracket of dQ -+ e, e = scale sum_j ddS_tj |k_jd| + (c_acc(32 nch) + 3) u32 scale sum_j |dS_tj k_jd|   (scale 2, product 1)
  dK     : the same with q and a sum over t
  dV     : bracket of dV -+ e, e = sum_t (u16 + eP_tj + c_acc(32 nch) u32) P_tj |dO_td|
  Every propagated sum is multiplied by 1 + 4 u16 for the products of two first-order terms.

Fallback (k_attention.hip; fp32 operands, bf16 only converts on the way in and out), per thread, keys in index order:
  eS_tj  = (HD + 3) u32 A_tj                 q * scale (scale 2, product 1), HD fmaf
  p      = __expf(sc - m_run): the subtraction and the argument scaling (log2e constant, product) 3 u32 |x|, |x| <= 2 max_j |S_tj| =: R_t
  a      = __expf(m - mn) multiplies o and l alike at every raise of the running maximum (it is exactly 1 otherwise: __expf(0)), and
             re-weights the earlier keys against the later ones: a key's weight carries its own p and every later a, whose arguments
             sum to <= R_t.  nr_t = the number of raises, counted on the reference's scores with 2 max eS of slack for near-ties.
           w_t = max_j eS_tj + 6 u32 R_t + (nr_t + 1) E_EXP      (relative error of a key's weight in o and in l)
  out    : e = (2 w_t + (2 T + 2 nr_t + 3) u32) sum_j P |v|  + u32 |O| for fp32 out / the bracket for bf16
             per key one fmaf into o and one into l, per raise the products o * a and l * a; inv and o * inv
  lse    : w_t + (T + nr_t + 2) u32 + (E_LOG + 2 u32) |log l| + u32 |lse|
  eP_tj  = HD u32 A_tj + 3 u32 |S_tj| + u32 |lse_t| + 4 u32 |S_tj - lse_t| + E_EXP      (sc * scale, the given lse, the subtraction, __expf)
  ddP    = HD u32 sum_d |dO v|;  dD_t = (HD u32 + u16 if bf16) sum_d |dO O|;  ddS = P (eP |dP - D| + ddP + dD) + 2 u32 |dS|
  dQ, dK : e = scale sum ddS |k| + (T + 3) u32 scale sum |dS k|;  dV: e = sum_t (eP + (T + 1) u32) P |dO|
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

from tests.gemm_ref import _bf16_key, _bracket, _key_to_double

U32 = 2.0 ** -24
U16 = 2.0 ** -8
E_EXP = 2.0 ** -23      # 1 ulp of the fp32 result (module docstring)
E_LOG = 2.0 ** -23
LOG2E = 1.4426950408889634
SECOND = 1 + 4 * U16    # products of two first-order terms
TINY = 2.0 ** -120      # flushed denormals of the raw exp2, far below any checked quantity
LDS_BYTES = 160 * 1024
FILL_BF16 = 0x7FD5      # NaNs with a payload: "still at the fill value" is told from a NaN that a kernel computed
FILL_F32 = 0x7FD5AAAA
HDS = (16, 24, 32, 48, 64)


def round_up(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------------------------------------ dispatch, restated
def attn_trims(chunks):
    return 1 <= chunks <= 3


def attn_image(T, Tp, row_stride, trim):
    rows = round_up(T, 16) if trim else Tp
    return rows, round_up(rows * row_stride, 1024)


def attn_fwd_lds(fq, img):
    return (2 if fq else 3) * img


def attn_bwd_lds(ph, img, Tp):
    return (4 if ph == 0 else 2) * img + 2 * Tp * 4


def attn_threads(T, max_threads):
    nt, maxw = (T + 15) // 16, max_threads // 64
    passes = (nt + maxw - 1) // maxw
    return 64 * ((nt + passes - 1) // passes)


def attn_supported(T, H, hd):
    return hd in (24, 32, 64) and 1 <= T <= 1024 and (H * hd) % 8 == 0


K_FWD_CAP = 512


def bwd_cap(nch):
    return 1024 if nch == 0 else 512


def _passes(T, threads):
    return -(-((T + 15) // 16) // (threads // 64))


@dataclass(frozen=True)
class Fwd:
    mfma: bool
    dtype: str
    HD: int
    nch_t: int = 0        # template NCH (0: runtime loop, online softmax)
    fq: bool = False
    padded: bool = False  # hdv < HD
    passes: int = 1       # tile passes of a wave (mfma) / query passes of a thread (generic)
    blocks: int = 1       # generic: LDS blocks of KB rows
    chunks: int = 1       # Tp / 32

    @property
    def label(self):
        if self.mfma:
            return (f"mfma<{self.HD},{self.nch_t},{'FQ' if self.fq else '-'}>", "pad" if self.padded else "-", f"passes={self.passes}")
        return (f"generic<{self.dtype},{self.HD}>", f"blocks={self.blocks}", f"qpasses={self.passes}")


@dataclass(frozen=True)
class Bwd:
    mfma: bool
    dtype: str
    HD: int
    nch_t: int = 0
    ph: int = 0           # 0: one launch; 12: the two launches PH = 1, PH = 2
    padded: bool = False
    passes: int = 1
    blocks: int = 1
    chunks: int = 1
    dform: str = "dO.O"   # "DPM": D = sum_j P dP in phase A; "dO.O" from the rounded out
    prologue: str = "-"   # "lse" (DPM: log-sum-exps only), "prefetch" (registers before the DMA wait), "loop" (plain)

    @property
    def label(self):
        if self.mfma:
            return (f"mfma<{self.HD},{self.nch_t},PH={'1+2' if self.ph else '0'}>", "pad" if self.padded else "-", f"passes={self.passes}",
                    self.dform, self.prologue)
        return (f"generic<{self.dtype},{self.HD}>", f"blocks={self.blocks}", f"qpasses={self.passes}", "dO.O", "-")


@dataclass(frozen=True)
class Route:
    fwd: Fwd
    bwd: Bwd

    @property
    def label(self):
        return self.fwd.label + ("|",) + self.bwd.label


def generic_block(T):
    return min(round_up(T, 64), 256)


def generic_kb(T, hd, backward):
    return min(T, (LDS_BYTES - (8 * T if backward else 0)) // (2 * hd * 4))


def _generic(cls, dtype, T, hd, backward):
    kb = generic_kb(T, hd, backward)
    return cls(False, dtype, hd, blocks=-(-T // kb), passes=-(-T // generic_block(T)))


def route_fwd(dtype, T, H, hd, aligned=True) -> Fwd:
    if dtype != "bf16" or not attn_supported(T, H, hd) or not aligned:
        return _generic(Fwd, dtype, T, hd, False)
    Tp, hdt = round_up(T, 32), 32 if hd == 24 else hd
    img = attn_image(T, Tp, hdt * 2 + 32, attn_trims(Tp >> 5))[1]
    threads = attn_threads(T, K_FWD_CAP)
    common = dict(padded=hd != hdt, passes=_passes(T, threads), chunks=Tp >> 5)
    if attn_fwd_lds(False, img) > LDS_BYTES:
        if attn_fwd_lds(True, img) > LDS_BYTES or hd != hdt:
            return _generic(Fwd, dtype, T, hd, False)
        return Fwd(True, dtype, hdt, 0, True, **common)
    return Fwd(True, dtype, hdt, Tp >> 5 if Tp >> 5 in (1, 2, 3, 5) else 0, False, **common)


def route_bwd(dtype, T, H, hd, aligned=True) -> Bwd:
    if dtype != "bf16" or not attn_supported(T, H, hd) or not aligned:
        return _generic(Bwd, dtype, T, hd, True)
    Tp, hdt = round_up(T, 32), 32 if hd == 24 else hd
    img = attn_image(T, Tp, hdt * 2 + 32, attn_trims(Tp >> 5))[1]
    if attn_bwd_lds(0, img, Tp) > LDS_BYTES:
        if attn_bwd_lds(1, img, Tp) > LDS_BYTES or hd != hdt:   # PH = 1 and PH = 2 ask for the same size
            return _generic(Bwd, dtype, T, hd, True)
        threads = attn_threads(T, bwd_cap(0))
        return Bwd(True, dtype, hdt, 0, 12, False, _passes(T, threads), chunks=Tp >> 5, dform="dO.O", prologue="loop")
    nch = Tp >> 5 if Tp >> 5 in (1, 2, 3) else 0
    threads = attn_threads(T, bwd_cap(nch))
    if nch:
        dform, prologue = "DPM", "lse"
    else:
        dform, prologue = "dO.O", "prefetch" if Tp * (hdt // 8) <= 4 * threads else "loop"
    return Bwd(True, dtype, hdt, nch, 0, hd != hdt, _passes(T, threads), chunks=Tp >> 5, dform=dform, prologue=prologue)


def route(dtype, T, H, hd, aligned=True) -> Route:
    return Route(route_fwd(dtype, T, H, hd, aligned), route_bwd(dtype, T, H, hd, aligned))


# A label one could write down from the kernel's template parameters that no shape selects, with the reason.
UNREACHABLE = {
    "mfma<*,0,PH=0> with the plain D loop":
        "needs Tp * HD / 8 > 4 * threads in one launch; threads = 64 waves with at most two 16-token tiles per wave whenever four images "
        "fit the LDS (Tp <= 224 at HD = 64: one tile per wave, 4 * threads >= 16 T - 240 >= 8 Tp; Tp <= 416 at HD = 32: at most two tiles "
        "per wave, 4 * threads >= 8 T - 120 >= 4 Tp for Tp >= 128), so the register-prefetched prologue always applies",
}


@lru_cache(None)
def universe():
    """Every route label that hd in HDS, 1 <= T <= 1024 and both dtypes can select -> the smallest (T, dtype, hd) that does.
    (H only enters through H hd % 8 == 0, which holds for every hd here; pointer alignment is a case of its own.)"""
    u = {}
    for dtype in ("bf16", "f32"):
        for hd in HDS:
            for T in range(1, 1025):
                u.setdefault(route(dtype, T, 2, hd).label, (T, dtype, hd))
    return u


@dataclass(frozen=True)
class Case:
    dtype: str
    B: int
    T: int
    H: int
    hd: int
    offset8: bool = False   # operand pointers 8 bytes past a 16-byte boundary
    why: str = ""

    @property
    def id(self):
        return f"{self.dtype}-B{self.B}-T{self.T}-H{self.H}-hd{self.hd}" + ("-off8" if self.offset8 else "")

    @property
    def route(self):
        return route(self.dtype, self.T, self.H, self.hd, not self.offset8)

    @property
    def label(self):
        return self.route.label + (f"BHmod8={self.B * self.H % 8}", "off8" if self.offset8 else "aligned")


CLASS_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 81, 96, 97, 128, 129, 145, 160, 161, 197, 257)
REMAP_BH = ((1, 1), (7, 1), (3, 3), (13, 1), (2, 8))   # B H = 1, 7, 9, 13, 16: remainders 1, 7, 1, 5, 0 of the XCD remap


@lru_cache(None)
def cases():
    out, seen = [], set()

    def add(c):
        if c.id not in seen:
            seen.add(c.id)
            out.append(c)

    for lbl, (T, dtype, hd) in universe().items():            # the smallest T of every route label: both sides of every threshold
        add(Case(dtype, 1, T, 2, hd, why="smallest T of its label"))
    for hd in (24, 32, 64):                                    # lengths inside each chunk class: tails, clamps, full chunks
        for T in CLASS_LENGTHS:
            add(Case("bf16", 2, T, 3, hd, why="chunk class"))
    for hd in (24, 32, 64):
        for T in (1, 17, 64, 145):
            add(Case("f32", 2, T, 3, hd, why="fallback lengths"))
    for B, H in REMAP_BH:                                      # att_block() with a remainder, in an unrolled and a chunk-loop kernel
        add(Case("bf16", B, 36, H, 64, why="XCD remap"))
        add(Case("bf16", B, 145, H, 32, why="XCD remap"))
    for dtype in ("bf16", "f32"):
        add(Case(dtype, 2, 36, 2, 32, offset8=True, why="misaligned operands"))
    for H in (1, 3):
        for T in (17, 36, 81):
            add(Case("bf16", 2, T, H, 24, why="hd = 24 heads"))
    return tuple(out)


def coverage_gaps(table=None):
    """Route labels of the universe without a case, remainders of the remap without an MFMA case, missing alignment cases."""
    table = cases() if table is None else table
    have = {c.route.label for c in table if not c.offset8}
    gaps = [("route", lbl) for lbl in universe() if lbl not in have]
    for kind in ("fwd", "bwd"):
        rem = {c.B * c.H % 8 for c in table if getattr(c.route, kind).mfma}
        gaps += [("remap", kind, r) for r in (0, 1, 5, 7) if r not in rem]
    for dtype in ("bf16", "f32"):
        if not any(c.offset8 and c.dtype == dtype and not c.route.fwd.mfma and not c.route.bwd.mfma for c in table):
            gaps.append(("offset8", dtype))
    for H in (1, 3):
        if not any(c.hd == 24 and c.H == H and c.route.fwd.padded for c in table):
            gaps.append(("hd24", H))
    return gaps


# ------------------------------------------------------------------------------------------------ reference
def split_heads(x, H, hd, parts=1):
    """(B, T, parts H hd) -> parts tensors (B, H, T, hd)."""
    B, T, _ = x.shape
    r = x.reshape(B, T, parts, H, hd).permute(2, 0, 3, 1, 4)
    return r[0] if parts == 1 else tuple(r.unbind(0))


def merge_heads(*xs):
    """(B, H, T, hd) tensors -> (B, T, len(xs) H hd)."""
    B, H, T, hd = xs[0].shape
    return torch.stack(xs, 0).permute(1, 3, 0, 2, 4).reshape(B, T, len(xs) * H * hd)


@dataclass
class Ref:
    hd: int
    q: torch.Tensor
    k: torch.Tensor
    v: torch.Tensor
    do: torch.Tensor
    S: torch.Tensor
    M: torch.Tensor
    P: torch.Tensor
    O: torch.Tensor
    lse: torch.Tensor
    dP: torch.Tensor
    D: torch.Tensor
    dS: torch.Tensor
    dQ: torch.Tensor
    dK: torch.Tensor
    dV: torch.Tensor

    @property
    def scale(self):
        return self.hd ** -0.5

    def backward_inputs(self, dtype):
        """(out, lse) as the backward is given them: the reference rounded to the activation type / to fp32."""
        return merge_heads(self.O).to(dtype), self.lse.float()


def reference(qkv, do, H, hd) -> Ref:
    q, k, v = (x.double() for x in split_heads(qkv, H, hd, 3))
    g = split_heads(do, H, hd).double()
    scale = hd ** -0.5
    S = scale * (q @ k.transpose(-1, -2))
    M = S.amax(-1)
    E = torch.exp(S - M[..., None])
    l = E.sum(-1)
    P = E / l[..., None]
    dP = g @ v.transpose(-1, -2)
    D = (P * dP).sum(-1)
    dS = P * (dP - D[..., None])
    return Ref(hd, q, k, v, g, S, M, P, P @ v, M + torch.log(l), dP, D, dS, scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q),
               P.transpose(-1, -2) @ g)


# ------------------------------------------------------------------------------------------------ bounds
def c_acc(K):
    return K // 32 + 1


def bounds_fwd(r: Ref, f: Fwd):
    """-> e_out (B, H, T, hd), e_lse (B, H, T): error allowed before the output rounding (module docstring)."""
    A = r.scale * (r.q.abs() @ r.k.abs().transpose(-1, -2))
    Pv = r.P @ r.v.abs()
    T = r.S.shape[-1]
    logl = (r.lse - r.M).abs()
    if f.mfma:
        nch = f.chunks
        online = f.nch_t == 0
        eS = (c_acc(f.HD) * U32 * A + 5 * U32 * r.S.abs() + 6 * U32 * r.M.abs()[..., None]).amax(-1)
        if online:
            eS = eS + nch * (E_EXP + 3 * U32 * r.S.abs().amax(-1))
        c = (8 * nch + 2) + 2 + c_acc(32 * nch) + 2 + (3 * nch if online else 0)
        e_out = (U16 + 2 * eS[..., None] + E_EXP + c * U32) * Pv * SECOND
        e_lse = (eS + 4 * U32 * r.M.abs() + U32 * logl + (8 * nch + 2) * U32 + E_EXP + (E_LOG + 2 * U32) * logl
                 + (2 * nch * U32 if online else 0))
    else:
        eS = ((f.HD + 3) * U32 * A).amax(-1)
        R = 2 * r.S.abs().amax(-1)
        prev = torch.cummax(r.S, -1).values[..., :-1]
        nr = 1 + (r.S[..., 1:] > prev - 2 * eS[..., None]).sum(-1)
        w = eS + 6 * U32 * R + (nr + 1) * E_EXP
        e_out = (2 * w + (2 * T + 2 * nr + 3) * U32)[..., None] * Pv * SECOND
        if f.dtype == "f32":
            e_out = e_out + U32 * r.O.abs()
        e_lse = w + (T + nr + 2) * U32 + (E_LOG + 2 * U32) * logl + U32 * r.lse.abs()
    return e_out + TINY, e_lse + TINY


def bounds_bwd(r: Ref, b: Bwd):
    """-> e_dq, e_dk, e_dv (B, H, T, hd).  The reference the outputs are compared with stays r.dQ, r.dK, r.dV: the rounding of the given
    out and lse is part of the bound (dD, eP)."""
    A = r.scale * (r.q.abs() @ r.k.abs().transpose(-1, -2))
    T = r.S.shape[-1]
    lse = r.lse.abs()[..., None]
    adP = r.do.abs() @ r.v.abs().transpose(-1, -2)
    dOO = (r.do.abs() * r.O.abs()).sum(-1)
    PdP = (r.P * r.dP.abs()).sum(-1)
    dmD = (r.dP - r.D[..., None]).abs()
    if b.mfma:
        nch = b.chunks
        eP = c_acc(b.HD) * U32 * A + 5 * U32 * r.S.abs() + 4 * U32 * lse * LOG2E + E_EXP
        ddP = c_acc(b.HD) * U32 * adP
        if b.dform == "DPM":
            dD = (r.P * (eP * r.dP.abs() + ddP)).sum(-1) + (8 * nch + 2) * U32 * PdP
        else:
            dD = (U16 + (8 + int(math.log2(b.HD // 8)) + 1) * U32) * dOO
        ddS = (U16 * r.dS.abs() + r.P * (eP * dmD + ddP + dD[..., None]) + 2 * U32 * r.dS.abs()) * SECOND + TINY * dmD
        c_out, c_dv, u_p = c_acc(32 * nch) + 3, c_acc(32 * nch), U16
    else:
        eP = b.HD * U32 * A + 3 * U32 * r.S.abs() + U32 * lse + 4 * U32 * (r.S - r.lse[..., None]).abs() + E_EXP
        ddP = b.HD * U32 * adP
        dD = (b.HD * U32 + (U16 if b.dtype == "bf16" else 0)) * dOO
        ddS = (r.P * (eP * dmD + ddP + dD[..., None]) + 2 * U32 * r.dS.abs()) * SECOND + TINY * dmD
        c_out, c_dv, u_p = T + 3, T + 1, 0.0
    s = r.scale
    e_dq = s * (ddS @ r.k.abs()) + c_out * U32 * s * (r.dS.abs() @ r.k.abs())
    e_dk = s * (ddS.transpose(-1, -2) @ r.q.abs()) + c_out * U32 * s * (r.dS.abs().transpose(-1, -2) @ r.q.abs())
    e_dv = (((u_p + eP + c_dv * U32) * r.P + TINY).transpose(-1, -2) @ r.do.abs()) * SECOND
    if b.dtype == "f32":
        e_dq, e_dk, e_dv = e_dq + U32 * r.dQ.abs(), e_dk + U32 * r.dK.abs(), e_dv + U32 * r.dV.abs()
    return e_dq + TINY, e_dk + TINY, e_dv + TINY


# ------------------------------------------------------------------------------------------------ report and checks
@dataclass
class Report:
    what: str
    n: int = 0
    bad: int = 0
    nan: int = 0
    fill: int = 0
    worst_ratio: float = 0.0
    worst: tuple = ()       # (image, head, token, column or None, got, ref, allowed distance)
    first_bad: tuple = ()   # (image, head, token, column or None)

    @property
    def ok(self):
        return self.n > 0 and self.bad == 0 and self.nan == 0 and self.fill == 0

    def __str__(self):
        s = f"{self.what}: {self.bad} of {self.n} outside the bound, {self.nan} NaN, {self.fill} at the fill value; worst error/bound {self.worst_ratio:.3g}"
        if self.worst:
            b, h, t, c, got, ref, bd = self.worst
            s += f" at (image {b}, head {h}, token {t}, column {c}; 16-token tile {t // 16}, 32-key chunk {t // 32}): got {got:.9g}, fp64 {ref:.9g}, allowed {bd:.3g}"
        if self.first_bad:
            b, h, t, c = self.first_bad
            s += f"; first failing element (image {b}, head {h}, token {t}, column {c}; tile {t // 16}, chunk {t // 32})"
        return s


def fill_like(shape, dtype, device="cpu"):
    """A buffer of NaNs with the fill payload."""
    if dtype == torch.bfloat16:
        return torch.full(shape, FILL_BF16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full(shape, FILL_F32, dtype=torch.int32, device=device).view(torch.float32)


def at_fill(x):
    if x.dtype == torch.bfloat16:
        return x.view(torch.int16) == FILL_BF16
    return x.view(torch.int32) == FILL_F32


GUARD = 256   # elements in front of and behind every output (a multiple of 16 bytes in either type)


def guarded(shape, dtype, device="cpu", offset=0):
    """A fill-valued flat buffer and the view of it that a kernel writes: GUARD + offset elements in front, GUARD behind."""
    n = math.prod(shape)
    buf = fill_like((GUARD + offset + n + GUARD,), dtype, device)
    return buf, buf[GUARD + offset:GUARD + offset + n].view(shape)


def guards_touched(buf, view, offset=0):
    """Number of guard elements that no longer hold the fill value."""
    n = view.numel()
    m = at_fill(buf)
    return int((~m[:GUARD + offset]).sum()) + int((~m[GUARD + offset + n:]).sum())


def check(what, got, ref, e, *, bracket=None) -> Report:
    """got: the kernel's output in its own dtype, shaped like ref (B, H, T[, hd]); ref, e (> 0) in fp64.
    bf16 outputs (bracket defaults to the dtype): got must lie between the largest bf16 <= ref - e and the smallest bf16 >= ref + e, that
    is, some real x within e of ref rounds to got in one direction or the other.  The ratio reported is the distance from ref to the
    nearest such x (to the open interval between got's two bf16 neighbours; 0 if ref lies inside it) over e: the share of e that
    the element needs beyond its output rounding.  fp32 outputs: |got - ref| <= e, ratio |got - ref| / e."""
    bracket = got.dtype == torch.bfloat16 if bracket is None else bracket
    fillm = at_fill(got)
    g = got.double()
    nan = torch.isnan(g) & ~fillm
    if bracket:
        safe = torch.where(torch.isfinite(g), g, torch.zeros_like(g)).to(torch.bfloat16)
        key = _bf16_key(safe)
        bad = (key < _bracket(ref - e, up=False)) | (key > _bracket(ref + e, up=True))
        dist = torch.maximum(ref - _key_to_double(key + 1), _key_to_double(key - 1) - ref).clamp_min(0)
        allowed = e + (_key_to_double(key + 1) - _key_to_double(key - 1)) / 2
    else:
        dist = (g - ref).abs()
        bad = dist > e
        allowed = e
    ratio = torch.where(nan | fillm | ~torch.isfinite(g), torch.zeros_like(dist), dist / e)
    bad = (bad | ~torch.isfinite(g)) & ~nan & ~fillm
    rep = Report(what, n=g.numel(), bad=int(bad.sum()), nan=int(nan.sum()), fill=int(fillm.sum()))

    def where(i):
        idx = []
        for d in reversed(g.shape):
            idx.append(i % d)
            i //= d
        idx = idx[::-1]
        return tuple(idx) if g.dim() == 4 else tuple(idx) + (None,)

    i = int(torch.nan_to_num(ratio, nan=float("inf"), posinf=float("inf")).flatten().argmax())
    rep.worst_ratio = float(ratio.flatten()[i])
    rep.worst = where(i) + (float(g.flatten()[i]), float(ref.flatten()[i]), float(allowed.flatten()[i]))
    anyfail = bad | nan | fillm
    if bool(anyfail.any()):
        rep.first_bad = where(int(anyfail.flatten().to(torch.int32).argmax()))
    return rep


def check_fwd(r: Ref, f: Fwd, out, lse, what=""):
    """out (B, T, H hd) in the activation type, lse (B, H, T) fp32 -> {"out": Report, "lse": Report}."""
    H = r.q.shape[1]
    e_out, e_lse = bounds_fwd(r, f)
    return {"out": check(f"{what} out", split_heads(out, H, r.hd), r.O, e_out),
            "lse": check(f"{what} lse", lse, r.lse, e_lse, bracket=False)}


def check_bwd(r: Ref, b: Bwd, d_qkv, what=""):
    H = r.q.shape[1]
    dq, dk, dv = split_heads(d_qkv, H, r.hd, 3)
    e_dq, e_dk, e_dv = bounds_bwd(r, b)
    return {"dQ": check(f"{what} dQ", dq, r.dQ, e_dq), "dK": check(f"{what} dK", dk, r.dK, e_dk), "dV": check(f"{what} dV", dv, r.dV, e_dv)}


def exact_mismatches(got, want):
    """Number of elements whose bits differ (-0 and +0 count as different; want is given in got's dtype)."""
    a, b = (x.view(torch.int16) if x.dtype == torch.bfloat16 else x.view(torch.int32) for x in (got.contiguous(), want.contiguous()))
    return int((a != b).sum())


# ------------------------------------------------------------------------------------------------ input families
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % 2147483647
    return torch.Generator().manual_seed(seed)


def gen_random(c: Case, sigma, dtype):
    g = _gen(1, c.B, c.T, c.H, c.hd, int(sigma))
    qkv = (sigma * torch.randn(c.B, c.T, 3 * c.H * c.hd, generator=g)).to(dtype)
    do = torch.randn(c.B, c.T, c.H * c.hd, generator=g).to(dtype)
    return qkv, do


def _nonzero_ints(shape, g):
    x = torch.randint(1, 128, shape, generator=g)
    return x * (2 * torch.randint(0, 2, shape, generator=g) - 1)


def gen_routing(c: Case, dtype):
    """K_j = +-16 by the low ceil(log2 T) bits of j, Q_t = K_sigma(t): query t puts all its weight on key sigma(t) (the next score is
    512 hd^-1/2 >= 64 nats lower, every other probability < e^-64).  V and dO are non-zero integers of magnitude <= 127: a zero would leave
    the e^-64 terms standing alone in an accumulator, and the outputs would not be exact.
    -> qkv, do, sigma (B, H, T), want_out = V[sigma], want_dv = dO[sigma^-1], lse_exact."""
    B, T, H, hd = c.B, c.T, c.H, c.hd
    g = _gen(2, B, T, H, hd)
    n = max(1, math.ceil(math.log2(T))) if T > 1 else 1
    a = 16.0
    j = torch.arange(T)
    bits = torch.zeros(T, hd)
    for b in range(n):
        bits[:, b] = torch.where((j >> b) & 1 == 1, a, -a)
    sigma = torch.stack([torch.stack([torch.randperm(T, generator=g) for _ in range(H)]) for _ in range(B)])   # (B, H, T)
    k = bits.expand(B, H, T, hd)
    q = torch.gather(k, 2, sigma[..., None].expand(B, H, T, hd))
    v = _nonzero_ints((B, H, T, hd), g).float()
    do = _nonzero_ints((B, H, T, hd), g).float()
    inv = torch.argsort(sigma, -1)
    want_out = torch.gather(v, 2, sigma[..., None].expand(B, H, T, hd))
    want_dv = torch.gather(do, 2, inv[..., None].expand(B, H, T, hd))
    return (merge_heads(q, k, v).to(dtype), merge_heads(do).to(dtype), sigma, merge_heads(want_out).to(dtype), want_dv.to(dtype),
            n * a * a / math.sqrt(hd))


def gen_counting(c: Case, dtype):
    """Q = 0 (every probability exactly 1 / T), V[j, d] = [j = d mod hd]: out[t, d] T is the number of keys j < T with j = d mod hd."""
    B, T, H, hd = c.B, c.T, c.H, c.hd
    g = _gen(3, B, T, H, hd)
    k = torch.randn(B, H, T, hd, generator=g)
    v = (torch.arange(T)[:, None] % hd == torch.arange(hd)[None, :]).float().expand(B, H, T, hd)
    count = v[0, 0].sum(0)                                   # (hd,)
    return merge_heads(torch.zeros(B, H, T, hd), k, v).to(dtype), count.double()


def check_counting(r: Ref, f: Fwd, out, lse, count, what="counting"):
    """out = count * fl(1 / T) in fp32 (an exact integer accumulator times one rounded reciprocal), then the output rounding:
    count / T within 2 fp32 ulps, bracketed in bf16.  lse = log T within the general bound (S = 0 and A = 0 leave its summation terms)."""
    T, H = r.S.shape[-1], r.q.shape[1]
    o = split_heads(out, H, r.hd)
    ref = (count.to(o.device) / T).expand(o.shape).contiguous()
    logT = torch.full(lse.shape, math.log(T), dtype=torch.float64, device=lse.device)
    return {"out": check(f"{what} out", o, ref, 2 * 2.0 ** -23 * ref), "lse": check(f"{what} lse", lse, logT, bounds_fwd(r, f)[1], bracket=False)}


# ------------------------------------------------------------------------------------------------ honest-kernel emulation (MFMA path)
def _f32(x):
    return x.float()


def _mm32(a, b):
    """a (.., M, K) @ b (.., K, N) as the MFMA accumulates it: exact products, one fp32 rounding of the running sum per 32-deep step."""
    K = a.shape[-1]
    acc = torch.zeros(a.shape[:-1] + (b.shape[-1],), dtype=torch.float32)
    for k0 in range(0, K, 32):
        acc = (acc.double() + a[..., k0:k0 + 32].double() @ b[..., k0:k0 + 32, :].double()).float()
    return acc


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def _pad_rows(x, Tp):
    """Rows T .. Tp - 1 read the last valid row (the staging DMA and the row clamps)."""
    T = x.shape[-2]
    return x if Tp == T else torch.cat([x, x[..., T - 1:T, :].expand(x.shape[:-2] + (Tp - T, x.shape[-1]))], -2)


def emulate_mfma(qkv, do, H, hd, *, online, dpm, out_in=None, lse_in=None, mut=None):
    """torch fp32 emulation of attn_fwd_mfma_kernel / attn_bwd_mfma_kernel on bf16 operands (CPU): fp32 sums of bf16 products, P and dS
    rounded to bf16 once, the two-pass (online = False) or the online softmax, D = sum_j P dP (dpm) or dO . O from the given out.
    mut (mutations for the tests of the checkers): {"unmask": True} keys past T keep their scores; {"d_shift": tile} the queries of one tile
    take the D of their neighbour; {"pv_swap": chunk} keys 4-7 and 16-19 of one chunk trade places in P V.
    -> out (bf16), lse (fp32), d_qkv (bf16)"""
    mut = mut or {}
    q, k, v = (_f32(x) for x in split_heads(qkv, H, hd, 3))
    g = _f32(split_heads(do, H, hd))
    T = q.shape[-2]
    Tp = round_up(T, 32)
    nch = Tp // 32
    scale = torch.tensor(1.0, dtype=torch.float32) / torch.sqrt(torch.tensor(float(hd), dtype=torch.float32))
    sl2 = scale * torch.tensor(LOG2E, dtype=torch.float32)
    kp, vp = _pad_rows(k, Tp), _pad_rows(v, Tp)
    s = _mm32(q, kp.transpose(-1, -2))                                     # (B, H, T, Tp) raw scores
    if not mut.get("unmask"):
        s[..., T:] = -float("inf")

    def pv(p, c):
        pb = p.bfloat16().float()
        if mut.get("pv_swap") == c:
            pb = pb.clone()
            a, b = pb[..., 4:8].clone(), pb[..., 16:20].clone()
            pb[..., 4:8], pb[..., 16:20] = b, a
        return pb.double() @ vp[..., c * 32:c * 32 + 32, :].double()

    oacc = torch.zeros_like(q)
    if not online:
        m = s.amax(-1)
        mn2 = m * sl2
        p = torch.exp2(_fma(s, sl2, -mn2[..., None]))
        lsum = p.sum(-1)
        for c in range(nch):
            oacc = (oacc.double() + pv(p[..., c * 32:c * 32 + 32], c)).float()
    else:
        m = torch.full(q.shape[:-1], -float("inf"))
        lsum = torch.zeros(q.shape[:-1])
        for c in range(nch):
            sc = s[..., c * 32:c * 32 + 32]
            mn = torch.maximum(m, sc.amax(-1))
            mn2 = mn * sl2
            alpha = torch.exp2(m * sl2 - mn2)
            p = torch.exp2(_fma(sc, sl2, -mn2[..., None]))
            lsum = lsum * alpha + p.sum(-1)
            oacc = ((oacc * alpha[..., None]).double() + pv(p, c)).float()
            m = mn
    out = merge_heads(oacc * (1.0 / lsum)[..., None]).bfloat16()
    lse = m * scale + torch.log(lsum)
    # ---- backward
    lse_g = lse if lse_in is None else lse_in
    o_g = split_heads(out if out_in is None else out_in, H, hd).float()
    li = lse_g * torch.tensor(LOG2E, dtype=torch.float32)
    P = torch.exp2(_fma(s, sl2, -li[..., None]))[..., :T]                  # (B, H, T, T); masked keys were -inf
    if mut.get("unmask"):
        Pfull = torch.exp2(_fma(s, sl2, -li[..., None]))
    G = _mm32(g, v.transpose(-1, -2))
    D = (P * G).sum(-1) if dpm else (g * o_g).sum(-1)
    if "d_shift" in mut:
        t0 = 16 * mut["d_shift"]
        D = D.clone()
        D[..., t0:t0 + 16] = torch.roll(D[..., t0:t0 + 16], 1, -1)
    dS = (P * (G - D[..., None])).bfloat16().float()
    Pb = P.bfloat16().float()
    dq = _mm32(dS, k) * scale
    dk = _mm32(dS.transpose(-1, -2), q) * scale
    dv = _mm32(Pb.transpose(-1, -2), g)
    if mut.get("unmask") and Tp > T:   # the padded keys take their share of dQ as well (K rows clamp to the last key)
        GP = _mm32(g, vp.transpose(-1, -2))
        dSf = (Pfull * (GP - D[..., None])).bfloat16().float()
        dq = _mm32(dSf, kp) * scale
    return out, lse, merge_heads(dq, dk, dv).bfloat16()
