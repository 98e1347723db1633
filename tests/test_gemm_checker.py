"""The per-element GEMM checker of tests/gemm_ref.py on the CPU: it accepts the output of a correct kernel, emulated as bf16
operands with fp32 accumulation in 64-deep steps, and rejects each fault a wrong tile loop or epilogue would leave behind.
Also on the CPU: the dispatch restatement's coverage of the -m gpu table, and the shipped ISA of the NT kernel against the
gfx950 store-data hazard of bstore16 (k_gemm_nt3.hip)."""
import os
import subprocess
from pathlib import Path

import pytest
import torch

from tests import gemm_ref as R

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "ssrl_vit_mae_jepa_amd" / "csrc"
M, N, K = 600, 384, 384            # ragged last tile row for 192- and 256-row tiles
BM, BN = 256, 192


def emulate(A, W, bias2d, aux, mode, f32, skip=None):
    """What a correct kernel computes: fp32 sums of 64-deep K-steps (each step's products summed exactly, then rounded),
    bias added in fp32, the epilogue on the fp32 value.  bias2d: (M, N) fp32 or None; skip = (rows, cols, step) leaves one
    K-step out of one region."""
    acc = torch.zeros(A.shape[0], W.shape[0], dtype=torch.float32)
    for s in range(K // 64):
        part = (A[:, 64 * s:64 * s + 64].double() @ W[:, 64 * s:64 * s + 64].double().t()).float()
        if skip is not None and skip[2] == s:
            part[skip[0], skip[1]] = 0
        acc = acc + part
    v = acc + bias2d if bias2d is not None else acc
    if mode in (R.NONE, R.KEEP):
        return v if f32 else v.bfloat16(), None
    if mode == R.MUL:
        return (v * aux.float()).bfloat16(), None
    c = v.bfloat16().double()
    act = R.gelu64(c).bfloat16()
    return (R.gelu_slope64(c).bfloat16(), act) if mode == R.GELU_GRAD else (act, None)


def operands(seed, bias=True, mode=R.NONE):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).bfloat16()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).bfloat16()
    b = torch.randn(N, generator=g) if bias else None
    aux = (torch.rand(M, N, generator=g) * 4 - 2).bfloat16() if mode == R.MUL else None
    return A, W, b, aux


VARIANTS = [(R.NONE, False, True), (R.NONE, False, False), (R.NONE, True, True), (R.NONE, True, False), (R.MUL, False, False),
            (R.MUL, False, True), (R.GELU_ACT, False, True), (R.GELU_GRAD, False, True), (R.GELU_GRAD, False, False)]
VID = [f"{R.MODE_NAME[m]}-{'f32' if f else 'bf16'}-{'b' if b else 'nb'}" for m, f, b in VARIANTS]


def _check(A, W, b, aux, mode, out, out2):
    return R.check_nt(A, W, b, aux, mode, out, out2, tile=(BM, BN), chunk_elems=1 << 16)


@pytest.mark.parametrize("mode,f32,bias", VARIANTS, ids=VID)
def test_clean_emulation_passes(mode, f32, bias):
    A, W, b, aux = operands(1, bias, mode)
    out, out2 = emulate(A, W, b[None].expand(M, N) if bias else None, aux, mode, f32)
    rep = _check(A, W, b, aux, mode, out, out2)
    assert rep.ok, str(rep)
    assert rep.n == M * N * (2 if mode == R.GELU_GRAD else 1)
    # a bound that could not tell a 2-ulp error from a correct result would show ratios far below 1
    if mode in (R.NONE, R.MUL) and not f32:
        assert rep.worst_ratio > 0.2, str(rep)
    if mode in (R.GELU_ACT, R.GELU_GRAD):   # half an ulp of the output rounding, at the nearest candidate pre-activation
        assert rep.worst_ratio <= 0.55, str(rep)


def _bump_ulps(t, r, c, n):
    k = R._bf16_key(t[r:r + 1, c:c + 1].clone()) + n
    t[r, c] = R._key_to_double(k).to(t.dtype)[0, 0]


FAULTS = ["2ulp", "store_hazard", "swap16", "bias_strip", "kstep", "fill"]


# 2 bf16 ulps: on the bf16 results of the plain and MUL epilogues (fp32 results carry the accumulation slack, GELU results
# the rounding interval of their pre-activation); the neighbouring bias strip: with a bias
FAULT_CASES = [(f, v) for f in FAULTS for v, vid in zip(VARIANTS, VID)
               if not (f == "2ulp" and (v[1] or v[0] in (R.GELU_ACT, R.GELU_GRAD))) and not (f == "bias_strip" and not v[2])]


@pytest.mark.parametrize("fault,variant", FAULT_CASES, ids=[f"{f}-{VID[VARIANTS.index(v)]}" for f, v in FAULT_CASES])
def test_injected_fault_is_caught(fault, variant):
    mode, f32, bias = variant
    A, W, b, aux = operands(2, bias, mode)
    b2d = b[None].expand(M, N).clone() if bias else None
    tm, tn = 1, 1                                                   # the faulty tile: rows 256..511, columns 192..383
    rows, cols = slice(tm * BM, (tm + 1) * BM), slice(tn * BN, (tn + 1) * BN)
    skip = None
    if fault == "bias_strip":
        b2d[rows, cols] = b[None, (tn - 1) * BN:tn * BN]               # the strip of the tile column to the left
    if fault == "kstep":
        skip = (rows, cols, 3)
    out, out2 = emulate(A, W, b2d, aux, mode, f32, skip)
    tgt = out2 if out2 is not None and fault in ("store_hazard", "fill") else out
    r0, c0 = tm * BM + 37, tn * BN + 8
    if fault == "2ulp":
        sub = out[rows, cols].float().abs()
        i = int(sub.flatten().argmax())                              # an element well away from zero
        _bump_ulps(out, tm * BM + i // BN, tn * BN + i % BN, 2)
    elif fault == "store_hazard":
        # dword 0 of one 16-byte store replaced by the dword of the lane 8 places away: in the paired whole-line store that
        # lane writes the same row 32 columns further on
        w = 2 if tgt.dtype == torch.bfloat16 else 1
        tgt[r0, c0:c0 + w] = tgt[r0, c0 + 32:c0 + 32 + w].clone()
    elif fault == "swap16":
        a, b_ = slice(tm * BM + 16, tm * BM + 32), slice(tm * BM + 32, tm * BM + 48)
        for t in (out, out2) if out2 is not None else (out,):
            x = t[a, cols].clone()
            t[a, cols] = t[b_, cols]
            t[b_, cols] = x
    elif fault == "fill":
        tgt[r0, c0] = float("nan")
    rep = _check(A, W, b, aux, mode, out, out2)
    assert not rep.ok, f"{fault} not caught: {rep}"
    assert rep.first_bad and rep.first_bad[0] // BM == tm and rep.first_bad[1] // BN == tn, str(rep)
    if fault == "fill":
        assert rep.nan == 1
    print(rep)


def test_fill_value_counted():
    A, W, b, aux = operands(3)
    out, _ = emulate(A, W, b[None].expand(M, N), None, R.NONE, True)
    out[5, 7] = -1234.5
    rep = R.check_nt(A, W, b, None, R.NONE, out, tile=(BM, BN), fill=-1234.5)
    assert rep.fill == 1 and not rep.ok


def test_bf16_neighbours():
    x = torch.tensor([1.0, -1.0, 0.0, 3.0e-3, -7.5, 1e-30], dtype=torch.float64)
    k = R._bf16_key(x.bfloat16())
    up, down = R._key_to_double(k + 1), R._key_to_double(k - 1)
    assert bool((up > x).all()) and bool((down < x).all())
    assert up[0] == 1 + 2 ** -7 and down[0] == 1 - 2 ** -8 and up[1] == -1 + 2 ** -8 and down[1] == -1 - 2 ** -7
    assert bool((R._key_to_double(R._bracket(x, up=False)) <= x).all()) and bool((R._key_to_double(R._bracket(x, up=True)) >= x).all())
    assert float(R.bf16_ulp(torch.tensor([1.0, 1.5, 0.75], dtype=torch.float64))[0]) == 2 ** -7


def test_wgrad_checker_catches_a_missing_row():
    g = torch.Generator().manual_seed(4)
    dY, A = torch.randn(5000, 192, generator=g).bfloat16(), torch.randn(5000, 128, generator=g).bfloat16()
    dW = (dY.double().t() @ A.double()).float()
    db = dY.double().sum(0).float()
    rep, repb = R.check_wgrad(dY, A, dW, db)
    assert rep.ok and repb.ok, (str(rep), str(repb))
    # the worst-case bound over a 5000-long reduction is loose (the -m gpu module adds integer operands, exact in fp32, for
    # single missing rows); a ragged tail of 3 rows counted -39 times lies beyond it
    bad = dW - (dY[-3:].double().t() @ A[-3:].double()).float() * 40
    assert not R.check_wgrad(dY, A, bad, db)[0].ok


def test_gpu_table_covers_the_dispatch():
    """The -m gpu table reaches every selectable (layout, mode, output dtype, bias) on a 256-CU device (asserted again there
    on the device's CU count)."""
    assert R.coverage_gaps(R.nt_cases(256), 256) == []
    labels = R.reachable_labels(256)
    assert {lbl[0] for lbl in labels} == {"<8,3,4>", "<12,2,8>", "<6,3,4>", "<6,4,4>", "<4,4,4>"}
    assert ("<12,2,8>", "77", "bf16", True) in labels and ("<6,4,4>", "none", "f32", False) in labels
    assert not any(lbl[0] == "<8,3,4>" and lbl[1] == "77" for lbl in labels)    # the 192 x 256 tiles keep non-temporal stores


def test_route_restates_the_dispatcher():
    r = R.nt3_route(290000, 192, 768, R.NONE, False, True, 256)
    assert (r.layout, r.mode, r.bm, r.bn, r.tiles, r.grid, r.a_nt) == ((12, 2, 8), R.NONE, 256, 192, 1133, 256, 1)
    r = R.nt3_route(72000, 384, 384, R.NONE, False, True, 256)
    assert (r.layout, r.mode, r.per_wg) == ((6, 3, 4), R.KEEP, 3)
    assert R.nt3_route(218000, 192, 192, R.NONE, True, True, 256).layout == (6, 4, 4)
    assert R.nt3_route(100, 192, 192, R.GELU_GRAD, True, True, 256) is None          # fp32 GELU outputs go to another kernel
    assert R.nt3_route(100, 192, 588, R.NONE, False, True, 256) is None              # K % 64
    assert R.nt3_route(1000, 576, 192, R.NONE, False, True, 256, R.Knobs(w2=True)).layout == (6, 4, 2)
    assert R.nt3_route(290000, 192, 768, R.NONE, False, True, 256, R.Knobs(bm=192)).layout == (6, 3, 4)


# ------------------------------------------------------------------------------------------------ shipped ISA
def test_nt3_buffer_stores_have_a_literal_zero_soffset(tmp_path):
    """bstore16 (k_gemm_nt3.hip) adds the scalar offset into the vector offset and leaves soffset = 0: with an SGPR soffset
    on a 128-bit store, the DPP move that builds the next store's data corrupts dword 0 of this one on gfx950 (timing-
    dependent wrong values in scattered rows).  Compiled with the Makefile's flags, every buffer_store_dword* of every
    gemm_nt3_kernel instantiation must carry the literal 0."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = tmp_path / "nt3.s"
    flags = [f.replace("$(ARCH)", "gfx950") for f in R.makefile_cxxflags(CSRC / "Makefile")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", str(CSRC / "k_gemm_nt3.hip"), "-o", str(asm)], check=True, cwd=CSRC,
                   capture_output=True, timeout=1200)
    bad, count = R.scan_nt3_stores(asm.read_text())
    assert len(count) > 0, "no gemm_nt3_kernel instantiation in the assembly"
    assert all(n > 0 for n in count.values()), [k for k, n in count.items() if n == 0]
    offenders = {k: v[:3] for k, v in bad.items() if v}
    assert not offenders, ("buffer stores with a non-zero soffset in gemm_nt3_kernel: the gfx950 store-data hazard described at "
                           f"bstore16 in k_gemm_nt3.hip is back ({sum(map(len, bad.values()))} stores): {offenders}")


def test_isa_scan_sees_a_scalar_soffset():
    asm = "\n".join(["_ZN3mae15gemm_nt3_kernelILi0EEEv: ; @x", "\tbuffer_store_dwordx4 v[96:99], v104, s[8:11], 0 offen",
                     "\tbuffer_store_dwordx4 v[96:99], v104, s[8:11], s12 offen", ".Lfunc_end0:", "\tbuffer_store_dword v1, v2, s[0:3], s4 offen"])
    bad, count = R.scan_nt3_stores(asm)
    assert count == {"_ZN3mae15gemm_nt3_kernelILi0EEEv": 2} and len(bad["_ZN3mae15gemm_nt3_kernelILi0EEEv"]) == 1
