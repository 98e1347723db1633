"""The GEMM kernels behind nt3 and the full-M ring, against fp64, element by element (-m gpu).

Everything launch_linear_fwd / launch_linear_wgrad can select besides the persistent nt3 kernel: gemm_nt_kernel (v1, three
instantiations), gemm_nt2_kernel (the epilogues nt3 declines), gemm_generic_kernel in its NT and TN stride layouts (bf16 and fp32
operands, split-K with atomics), gemm_tn_kernel (five instantiations, M-splits, slab_reduce_kernel) and colsum_kernel, at the
smallest shapes at which each can still go wrong (tests/gemm_ref.py fallback_fwd_cases / fallback_wgrad_cases).  Every case runs
twice back to back without a synchronisation into NaN-filled outputs with guard rows behind the last row: the guard rows must
stay NaN, nothing inside may be NaN, launch 2 must give the bits of launch 1 (except on the one route whose atomics have no
fixed order), and every element must lie inside the bound gemm_ref derives from that kernel's own summation.  Every case runs on
random data and on small integers, where every partial sum is exact in fp32 and the result is determined bit for bit.  The case
ids carry the route label the dispatch restatement predicts."""
import os
import zlib

import pytest
import torch

from tests import gemm_ref as R
from tests.util import BF16, F32, check, lib, stream, _ptr

pytestmark = pytest.mark.gpu


def _num_cus():
    try:
        if torch.cuda.is_available():
            return torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        pass
    return 256   # collection on a host without a GPU (the tests are skipped there)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int16)


NUM_CUS = _num_cus()

GUARD = 256     # rows behind the output: the tallest tile of these kernels
FWD_CASES = R.fallback_fwd_cases(NUM_CUS)
WGRAD_CASES = R.fallback_wgrad_cases()
WORST = {}      # route label -> {"random" | "int": (worst error / bound, case id)}
COUNT = {}      # route label -> cases run


def _note(label, run, rep, cid):
    w = WORST.setdefault(label, {})
    if run not in w or rep.worst_ratio > w[run][0]:
        w[run] = (rep.worst_ratio, cid)


class _Env:
    """One environment variable for the calls inside (the dispatchers read MAE_GEMM_NT / MAE_WGRAD per call), restored after."""

    def __init__(self, var, value):
        self.var, self.value = var, value

    def __enter__(self):
        self.saved = os.environ.get(self.var)
        if self.value is not None:
            os.environ[self.var] = self.value
        else:
            os.environ.pop(self.var, None)

    def __exit__(self, *a):
        if self.saved is None:
            os.environ.pop(self.var, None)
        else:
            os.environ[self.var] = self.saved


@pytest.fixture(autouse=True)
def _free():
    yield
    torch.cuda.empty_cache()


def _operand(shape, dev, g, integer, dtype, scale=1.0):
    if integer:
        return torch.randint(-3, 4, shape, device=dev, generator=g).to(dtype)
    return (torch.randn(shape, device=dev, generator=g) * scale).to(dtype)


def test_table_reaches_every_fallback_route():
    """Every reachable (label, mode, output type, bias) / (label, operand type, db) and every edge of fallback_coverage_gaps, on this
    device's CU count; generic_tn_splitk is the only route without a fixed summation order."""
    assert R.fallback_coverage_gaps(FWD_CASES + WGRAD_CASES, NUM_CUS) == []
    unordered = {c.route(NUM_CUS).label for c in FWD_CASES + WGRAD_CASES if not c.route(NUM_CUS).ordered}
    assert unordered == {"generic_tn_splitk"}


def test_table_holds_every_launch_the_nt3_table_drops():
    """Each engine launch nt_cases skips is in this table with its own (N, K, mode, output type, bias) at a small M, among them the
    ViT-L/14 patch embed; its weight gradient's widths and its split-K route are here too."""
    have = {(c.N, c.K, c.mode, c.f32, c.bias) for c in FWD_CASES if c.dt == "bf16" and c.sel is None and not c.misalign and c.M <= 1024}
    dropped = R.dropped_engine_launches(NUM_CUS)
    assert dropped and all(row[2:] in have for row in dropped), [row for row in dropped if row[2:] not in have]
    assert (1024, 588, R.NONE, True, True) in have
    assert any((c.N, c.K, c.dt) == (1024, 588, "bf16") and c.route().label == "generic_tn" for c in WGRAD_CASES)
    assert R.wgrad_route(25600, 1024, 588, "bf16", True).label == "generic_tn_splitk"
    assert any(c.K == 588 and c.dt == "bf16" and c.route().label == "generic_tn_splitk" for c in WGRAD_CASES)


def run_fwd_case(case, dev, integer):
    route = case.route(NUM_CUS)
    assert route.label == case.name, f"{case.id}: the dispatch restatement sends this call to {route.label}"
    M, N, K = case.M, case.N, case.K
    dt = torch.bfloat16 if case.dt == "bf16" else torch.float32
    odt = torch.float32 if case.f32 else torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(f"{case.id}{integer}".encode()))
    A = _operand((M, K), dev, g, integer, dt)
    W = _operand((N, K), dev, g, integer, dt, K ** -0.5)
    bias = bias_buf = None
    if case.bias:
        bias_buf = _operand((N + 4,), dev, g, integer, torch.float32)
        bias = bias_buf[1:N + 1] if case.misalign else bias_buf[:N]     # a view one float off 16-byte alignment
        assert (bias.data_ptr() % 16 != 0) == case.misalign
    aux = None
    if case.mode == R.MUL:
        aux = _operand((M, N), dev, g, integer, odt) if integer else (torch.rand(M, N, device=dev, generator=g) * 4 - 2).to(odt)
    elif case.mode == R.DGELU:
        aux = _operand((M, N), dev, g, integer, odt, 1.5).clamp_(-7, 7)
    elif case.mode == R.RESID:
        aux = _operand((M, N), dev, g, integer, torch.float32)
    two = case.mode in (R.GELU, R.GELU_GRAD)
    outs = [torch.full((M + GUARD, N), float("nan"), dtype=odt, device=dev) for _ in range(2)]
    outs2 = [torch.full((M + GUARD, N), float("nan"), dtype=odt, device=dev) for _ in range(2)] if two else [None] * 2
    with _Env("MAE_GEMM_NT", case.sel):
        for o, o2 in zip(outs, outs2):   # no synchronisation in between
            check(lib.mae_linear_fwd(_ptr(A), _ptr(W), _ptr(bias) if bias is not None else None, M, N, K, BF16 if case.dt == "bf16" else F32,
                                     case.mode, F32 if case.f32 else BF16, _ptr(o), _ptr(o2) if two else None,
                                     _ptr(aux) if aux is not None else None, stream(dev)))
    torch.cuda.synchronize()
    for i, o in enumerate(outs + [x for x in outs2 if x is not None]):
        assert R.guard_intact(o, M), f"{case.id}: launch {i % 2 + 1} wrote guard rows behind row {M - 1}"
    assert torch.equal(_bits(outs[1][:M]), _bits(outs[0][:M])), f"{case.id}: launch 2 differs from launch 1"
    if two:
        assert torch.equal(_bits(outs2[1][:M]), _bits(outs2[0][:M])), f"{case.id}: launch 2 (out2) differs from launch 1"
    rep = R.check_nt(A, W, bias, aux, case.mode, outs[0][:M], outs2[0][:M] if two else None, tile=route.tile, roundings=route.roundings,
                     gelu=route.gelu, what=f"{case.id} {'int' if integer else 'random'}")
    print(rep)
    _note(route.label, "int" if integer else "random", rep, case.id)
    assert rep.ok, str(rep)
    if integer:
        want = R.exact_forward(A, W, bias, aux, case.mode, case.f32)
        if want is not None:
            got = outs[0][:M].double()
            assert torch.equal(got, want), f"{case.id}: {int((got != want).sum())} elements differ from the exact result, first at {(got != want).nonzero()[0].tolist()}"


@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c.id)
def test_fallback_nt_matches_fp64_per_element(dev, case):
    run_fwd_case(case, dev, integer=False)
    run_fwd_case(case, dev, integer=True)
    COUNT[case.name] = COUNT.get(case.name, 0) + 1


def run_wgrad_case(case, dev, integer):
    M = case.M
    dt = torch.bfloat16 if case.dt == "bf16" else torch.float32
    probs = [(case.N, case.K)] + ([case.pair] if case.pair else [])
    routes = [R.wgrad_route(M, N, K, case.dt, case.db, True, case.sel, num_cus=NUM_CUS) for N, K in probs]
    assert routes[0].label == case.name, f"{case.id}: the dispatch restatement sends this call to {routes[0].label}"
    g = torch.Generator(device=dev).manual_seed(zlib.crc32(f"{case.id}{integer}".encode()))
    ops = [(_operand((M, N), dev, g, integer, dt), _operand((M, K), dev, g, integer, dt)) for N, K in probs]
    nbytes = lib.mae_linear_wgrad_pair_scratch_bytes(M, *probs[0], *probs[1]) if case.pair else lib.mae_linear_wgrad_scratch_bytes(M, *probs[0])
    scratch = torch.full((max(256, nbytes),), 255, dtype=torch.uint8, device=dev)    # NaN bit patterns: a slab read before it is written shows
    runs = []
    with _Env("MAE_WGRAD", case.sel):
        for _ in range(2):   # no synchronisation in between
            outs = [(torch.full((N + GUARD, K), float("nan"), device=dev), torch.full((N + 64,), float("nan"), device=dev) if case.db else None)
                    for N, K in probs]
            if case.pair:
                (y0, a0), (y1, a1) = ops
                check(lib.mae_linear_wgrad_pair(_ptr(y0), _ptr(a0), *probs[0], _ptr(outs[0][0]), _ptr(outs[0][1]), _ptr(y1), _ptr(a1), *probs[1],
                                                _ptr(outs[1][0]), _ptr(outs[1][1]), M, BF16, _ptr(scratch), stream(dev)))
            else:
                check(lib.mae_linear_wgrad(_ptr(ops[0][0]), _ptr(ops[0][1]), M, *probs[0], BF16 if case.dt == "bf16" else F32, _ptr(outs[0][0]),
                                           _ptr(outs[0][1]) if case.db else None, _ptr(scratch), stream(dev)))
            runs.append(outs)
    torch.cuda.synchronize()
    run = "int" if integer else "random"
    for (N, K), (dY, A), route, (dW, db), (dW2, db2) in zip(probs, ops, routes, runs[0], runs[1]):
        name = f"{case.id} {N}x{K} {run}"
        for t in (dW, dW2):
            assert R.guard_intact(t, N), f"{name}: rows behind row {N - 1} of dW written"
        for t in (db, db2) if case.db else ():
            assert R.guard_intact(t, N), f"{name}: elements behind db[{N - 1}] written"
        if route.ordered or integer:   # atomics in no fixed order: equal bits only where every partial sum is exact
            assert torch.equal(_bits(dW[:N]), _bits(dW2[:N])), f"{name}: launch 2 differs from launch 1"
            assert not case.db or torch.equal(_bits(db[:N]), _bits(db2[:N])), f"{name}: launch 2 (db) differs from launch 1"
        for w, b in ((dW, db), (dW2, db2)) if not route.ordered else ((dW, db),):
            rep, repb = R.check_wgrad(dY, A, w[:N], b[:N] if case.db else None, what=name, roundings=route.roundings,
                                      db_roundings=route.db_roundings, tile=route.tile)
            print(rep, repb if repb is not None else "")
            _note(route.label, run, rep, case.id)
            if repb is not None:
                _note(("colsum " + case.dt) if route.colsum else route.label + " db", run, repb, case.id)
            assert rep.ok, str(rep)
            assert repb is None or repb.ok, str(repb)
            if integer:
                ref = dY.double().t() @ A.double()
                assert torch.equal(w[:N].double(), ref), f"{name}: dW differs from the exact sum at {int((w[:N].double() != ref).sum())} elements"
                assert not case.db or torch.equal(b[:N].double(), dY.double().sum(0)), f"{name}: db differs from the exact sum"


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: c.id)
def test_fallback_wgrad_matches_fp64_per_element(dev, case):
    run_wgrad_case(case, dev, integer=False)
    run_wgrad_case(case, dev, integer=True)
    COUNT[case.name] = COUNT.get(case.name, 0) + 1


def test_zz_report():
    """Prints route -> cases in the table / run here, and the worst error / bound per route on the random and the integer runs."""
    table = {}
    for c in FWD_CASES + WGRAD_CASES:
        table[c.name] = table.get(c.name, 0) + 1
    print(f"\nfallback GEMM routes on {NUM_CUS} CUs: route, cases in the table, cases run, worst error / bound (random | integer)")
    for lbl in sorted(set(table) | set(WORST)):
        w = WORST.get(lbl, {})
        cell = lambda k: f"{w[k][0]:.3f} ({w[k][1]})" if k in w else "-"   # noqa: E731
        print(f"  {lbl:22s} {table.get(lbl, 0):4d} {COUNT.get(lbl, 0):4d}  {cell('random')} | {cell('int')}")
