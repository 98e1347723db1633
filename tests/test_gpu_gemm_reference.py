"""NT and wgrad GEMMs against fp64, element by element, at the shapes the engine issues (-m gpu).

Every NT launch of the ViT-S/8 (B = 2000, 192- and 512-wide decoders), ViT-B/16 (B = 512) and ViT-L/14 I-JEPA (B = 256)
steps, forward and dgrad, with the edges of the persistent grid, runs three times back to back into NaN-filled outputs with
guard rows behind row M - 1: launches 2 and 3 must equal launch 1 bit for bit, the guard rows must stay untouched, and every
element must lie inside the bound of tests/gemm_ref.py around the fp64 result.  A restatement of the dispatcher labels every
case with its (layout, mode, output dtype, bias); the table must reach every label the dispatcher can select.  The tile
heights / widths chosen once per process (MAE_NT_BM, MAE_NT_WN1, MAE_NT_N256) are forced in child processes.  The wgrad
kernels run at the engine's full M, on random data (per-element bound) and on small integers (exact in fp32: bit-equal to fp64)."""
import json
import os
import subprocess
import sys
import zlib
from pathlib import Path

import pytest
import torch

from tests import gemm_ref as R
from tests.util import BF16, F32, check, lib, stream, _ptr

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
GUARD = 512   # rows behind the output (a 256-row tile may start up to 255 rows before the end)


def _num_cus():
    try:
        if torch.cuda.is_available():
            return torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass
    return 256   # collection on a host without a GPU (the tests are skipped there)


NUM_CUS = _num_cus()
CASES = R.nt_cases(NUM_CUS)
WORST = {}    # layout -> (worst error / bound, case id)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


def run_nt_case(case, dev, knobs=None):
    """Three back-to-back launches of one case; returns (route, report).  Asserts bit-identity and untouched guard rows."""
    knobs = R.Knobs.from_env() if knobs is None else knobs
    route = case.route(NUM_CUS, knobs)
    assert route is not None, case.id
    M, N, K = case.M, case.N, case.K
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(case.id.encode()))
    A = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    W = (torch.randn(N, K, device=dev, generator=g) / K ** 0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g) if case.bias else None
    aux = (torch.rand(M, N, device=dev, generator=g) * 4 - 2).to(torch.bfloat16) if case.mode == R.MUL else None
    odt = torch.float32 if case.f32 else torch.bfloat16
    two = case.mode == R.GELU_GRAD
    outs = [torch.full((M + GUARD, N), float("nan"), dtype=odt, device=dev) for _ in range(3)]
    outs2 = [torch.full((M + GUARD, N), float("nan"), dtype=odt, device=dev) for _ in range(3)] if two else [None] * 3
    saved = os.environ.get("MAE_GEMM_NT")
    if case.w2:
        os.environ["MAE_GEMM_NT"] = "v3w2"
    try:
        for o, o2 in zip(outs, outs2):   # no synchronisation in between: stages and stores of one launch in flight at the next
            check(lib.mae_linear_fwd(_ptr(A), _ptr(W), _ptr(bias) if bias is not None else None, M, N, K, BF16, case.mode,
                                     F32 if case.f32 else BF16, _ptr(o), _ptr(o2) if two else None, _ptr(aux) if aux is not None else None,
                                     stream(dev)))
    finally:
        if saved is None:
            os.environ.pop("MAE_GEMM_NT", None)
        else:
            os.environ["MAE_GEMM_NT"] = saved
    torch.cuda.synchronize()
    for i, o in enumerate(outs + [x for x in outs2 if x is not None]):
        assert bool(torch.isnan(o[M:]).all()), f"{case.id}: launch {i % 3 + 1} wrote guard rows behind row {M - 1}"
    for i in (1, 2):
        assert torch.equal(_bits(outs[i][:M]), _bits(outs[0][:M])), f"{case.id}: launch {i + 1} differs from launch 1"
        if two:
            assert torch.equal(_bits(outs2[i][:M]), _bits(outs2[0][:M])), f"{case.id}: launch {i + 1} (out2) differs from launch 1"
    rep = R.check_nt(A, W, bias, aux, case.mode, outs[0][:M], outs2[0][:M] if two else None, tile=(route.bm, route.bn),
                     what=f"{case.id} {R.LAYOUTS[route.layout]} mode {R.MODE_NAME[route.mode]}")
    return route, rep


def _note(route, rep, case_id):
    lay = R.LAYOUTS[route.layout]
    if lay not in WORST or rep.worst_ratio > WORST[lay][0]:
        WORST[lay] = (rep.worst_ratio, case_id)


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def test_table_reaches_every_selectable_instantiation():
    """Every (layout, mode, output dtype, bias) of the default dispatch and of MAE_GEMM_NT=v3w2, the production layouts at
    several tiles per workgroup and with column-changing workgroups, tile counts num_cus - 1 / num_cus / num_cus + 1, one-column
    grids for N = 128 / 192 / 256, M = 1 and ragged last tile rows: asserted on this device's CU count."""
    assert R.coverage_gaps(CASES, NUM_CUS) == []


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.id)
def test_nt_gemm_matches_fp64_per_element(dev, case):
    route, rep = run_nt_case(case, dev)
    _note(route, rep, case.id)
    assert rep.ok, str(rep)


def _child():
    """Entry point of a child process: the ViT-S/8 encoder and decoder launches under the tile knobs of its environment."""
    dev = torch.device("cuda:0")
    knobs = R.Knobs.from_env()
    seen = set()
    for name, M, N, K, mode, f32, bias in R.engine_launches(R.NETS[0], part=("enc", "dec")):
        case = R.Case(name, M, N, K, mode, f32, bias)
        if (M, N, K, mode, f32, bias) in seen:
            continue
        seen.add((M, N, K, mode, f32, bias))
        route, rep = run_nt_case(case, dev, knobs)
        print(json.dumps({"case": case.id, "label": route.label, "ratio": rep.worst_ratio, "ok": rep.ok, "per_wg": route.per_wg}), flush=True)
        if not rep.ok:
            print(str(rep), flush=True)
            sys.exit(1)
        del rep
        torch.cuda.empty_cache()
    print("child ok", flush=True)


FORCED = [{"MAE_NT_BM": "192"}, {"MAE_NT_BM": "256"}, {"MAE_NT_WN1": "0"}, {"MAE_NT_N256": "0"}]


def test_forced_tile_layouts_in_child_processes():
    """MAE_NT_BM=192|256, MAE_NT_WN1=0 and MAE_NT_N256=0 are read once per process: each runs the ViT-S/8 encoder and decoder
    launches in a fresh child (own time limit; no further child after a failure)."""
    script = f"import sys; sys.path.insert(0, {str(ROOT)!r}); from tests.test_gpu_gemm_reference import _child; _child()"
    for knob in FORCED:
        env = {k: v for k, v in os.environ.items() if not k.startswith("MAE_NT") and k != "MAE_GEMM_NT"}
        env.update(knob)
        r = subprocess.run([sys.executable, "-c", script], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "child ok" in r.stdout, f"{knob}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
        labels = set()
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                d = json.loads(line)
                labels.add(tuple(d["label"][:3]))
                lay = d["label"][0]
                if lay not in WORST or d["ratio"] > WORST[lay][0]:
                    WORST[lay] = (d["ratio"], f"{d['case']} {knob}")
        print(knob, sorted(labels), flush=True)
        if knob == {"MAE_NT_BM": "256"}:
            assert ("<12,2,8>", "none", "bf16") in labels and ("<12,2,8>", "77", "bf16") in labels
        if knob == {"MAE_NT_BM": "192"}:
            assert ("<6,3,4>", "none", "bf16") in labels
        if knob == {"MAE_NT_WN1": "0"}:
            assert ("<6,4,4>", "none", "bf16") in labels and not any(lbl[0] == "<12,2,8>" for lbl in labels)
        if knob == {"MAE_NT_N256": "0"}:
            assert not any(lbl[0] == "<8,3,4>" for lbl in labels)


# ----------------------------------------------------------------------------------------------- wgrad
def _rand(shape, dev, g, integer):
    if integer:   # small integers: every partial sum of an M-long reduction is exact in fp32 (|sum| <= 9 M < 2^24)
        return torch.randint(-3, 4, shape, device=dev, generator=g).to(torch.bfloat16)
    return torch.randn(shape, device=dev, generator=g).to(torch.bfloat16)


def _check_wgrad_outputs(name, dY, A, dW, db, integer):
    if integer:
        ref = dY.double().t() @ A.double()
        assert torch.equal(dW.double(), ref), f"{name}: dW differs from the exact sum at {int((dW.double() != ref).sum())} elements"
        assert torch.equal(db.double(), dY.double().sum(0)), f"{name}: db differs from the exact sum"
        return
    rep, repb = R.check_wgrad(dY, A, dW, db, what=name)
    lay = "wgrad"
    for r in (rep, repb):
        if lay not in WORST or r.worst_ratio > WORST[lay][0]:
            WORST[lay] = (r.worst_ratio, name)
    assert rep.ok, str(rep)
    assert repb.ok, str(repb)


@pytest.mark.parametrize("integer", [False, True], ids=["randn", "int"])
@pytest.mark.parametrize("name,M,s0,s1", R.wgrad_pairs(), ids=[p[0].replace(" ", "_") for p in R.wgrad_pairs()])
def test_wgrad_pair_matches_fp64_at_full_M(dev, name, M, s0, s1, integer):
    """mae_linear_wgrad_pair (a block's fc2 + fc1, proj + qkv in one launch) at the engine's row count; a second launch gives
    the same bits."""
    if integer:
        M += 77   # and a ragged tail in the last M-split
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(f"{name}{M}".encode()))
    ops = [(_rand((M, N), dev, g, integer), _rand((M, K), dev, g, integer), N, K) for N, K in (s0, s1)]
    scratch = torch.empty(lib.mae_linear_wgrad_pair_scratch_bytes(M, *s0, *s1), dtype=torch.uint8, device=dev)
    runs = []
    for _ in range(2):
        outs = [(torch.full((N, K), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev)) for _, _, N, K in ops]
        (y0, a0, N0, K0), (y1, a1, N1, K1) = ops
        check(lib.mae_linear_wgrad_pair(_ptr(y0), _ptr(a0), N0, K0, _ptr(outs[0][0]), _ptr(outs[0][1]), _ptr(y1), _ptr(a1), N1, K1,
                                        _ptr(outs[1][0]), _ptr(outs[1][1]), M, BF16, _ptr(scratch), stream(dev)))
        runs.append(outs)
    torch.cuda.synchronize()
    for (w, b), (w2, b2) in zip(runs[0], runs[1]):
        assert torch.equal(_bits(w), _bits(w2)) and torch.equal(_bits(b), _bits(b2)), f"{name}: second launch differs"
    for (dY, A, N, K), (dW, db) in zip(ops, runs[0]):
        _check_wgrad_outputs(f"{name} M={M} {N}x{K}", dY, A, dW, db, integer)


@pytest.mark.parametrize("integer", [False, True], ids=["randn", "int"])
@pytest.mark.parametrize("name,M,N,K", R.wgrad_singles(), ids=[p[0].replace(" ", "_") for p in R.wgrad_singles()])
def test_wgrad_matches_fp64_at_full_M(dev, name, M, N, K, integer):
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(f"{name}{M}".encode()))
    dY, A = _rand((M, N), dev, g, integer), _rand((M, K), dev, g, integer)
    scratch = torch.empty(lib.mae_linear_wgrad_scratch_bytes(M, N, K), dtype=torch.uint8, device=dev)
    dW = torch.full((N, K), float("nan"), device=dev)
    db = torch.full((N,), float("nan"), device=dev)
    check(lib.mae_linear_wgrad(_ptr(dY), _ptr(A), M, N, K, BF16, _ptr(dW), _ptr(db), _ptr(scratch), stream(dev)))
    torch.cuda.synchronize()
    _check_wgrad_outputs(f"{name} M={M} {N}x{K}", dY, A, dW, db, integer)


def test_zz_report():
    """Prints the coverage table (layout x mode x output dtype x bias) and the worst error / bound seen per layout."""
    cov = R.coverage(CASES, NUM_CUS)
    print(f"\nNT coverage on {NUM_CUS} CUs ({len(CASES)} cases): label -> cases, most tiles per workgroup")
    for lbl in sorted(cov, key=str):
        v = cov[lbl]
        print(f"  {lbl[0]:9s} {lbl[1]:9s} {lbl[2]:4s} bias={int(lbl[3])}  {len(v):3d}  {max(r.per_wg for _, r in v)}")
    print("worst error / bound per layout:")
    for lay, (ratio, cid) in sorted(WORST.items()):
        print(f"  {lay:9s} {ratio:.3e}  ({cid})")
