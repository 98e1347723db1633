"""Cost of a linear-probe sweep step against G serial probe steps, printed as one JSON document.

At (B, D, C) = (2000, 384, 10) and (16384, 1024, 100), for G = 1, 8 and 32 heads, in one process and with the same device events:
  * `ProbeSweep.step` (one BatchNorm, one mae_probe_sweep_head, two mae_lars_step_groups);
  * the yardstick a user had before: `LinearProbe.step` looped G times;
  * `mae_probe_sweep_head` alone (forward, softmax, weight gradient and its second stage), with the fp32 rate of its two GEMMs
    (4 B D G C flop);
  * the two GEMMs through `torch.mm` on the same operands (logits = y W_all^T and dW_all = dlogits^T y), fp32 without TF32.
Every figure is the median of `--repeats` windows; the windows of the cases alternate (case 1, 2, 3, 4, case 1, ...), so a drift of the
clocks falls on all of them alike.  No threshold: the table says where the sweep is faster and where it is not.

    python tools/probe_sweep_bench.py --out profiles/r29_probe_sweep_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from classifier_bench import timed  # noqa: E402
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.probe import LinearProbe, ProbeSweep, probe_lr  # noqa: E402

SHAPES = [(2000, 384, 10), (16384, 1024, 100)]
HEADS = (1, 8, 32)
SWEEP_LAUNCHES = 5 + 5 + 3 + 1   # BatchNorm; forward, softmax, reduce, weight gradient, its second stage; LARS on W; LARS on b


def bench(B, D, C, G, steps, warmup, repeats, dev) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(B, D, device=dev, generator=g) * 2 + 3
    labels = torch.randint(0, C, (B,), device=dev, generator=g)
    grid = [dict(base_learning_rate=0.01 * (i + 1), weight_decay=0.0005 * (i % 2)) for i in range(G)]
    sweep = ProbeSweep(D, C, grid, device=dev)
    probe = LinearProbe(D, C, device=dev)
    lr = probe_lr(probe.cfg)
    lib, stream = _lib.lib, torch.cuda.current_stream(dev).cuda_stream
    y = torch.randn(B, D, device=dev, generator=g)
    need = lib.mae_probe_sweep_scratch_bytes(B, D, C, G)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    loss, correct = torch.empty(G, device=dev), torch.empty(G, dtype=torch.int32, device=dev)
    hg = torch.empty_like(sweep.flat)
    w_all = torch.randn(G * C, D, device=dev, generator=g) * 0.01
    dl = torch.randn(B, G * C, device=dev, generator=g) / B

    def looped():
        for _ in range(G):
            probe.step(feats, labels, lr)

    def head():
        _lib.check(lib.mae_probe_sweep_head(y.data_ptr(), B, D, sweep.flat.data_ptr(), G, C, labels.data_ptr(), None, loss.data_ptr(),
                                            correct.data_ptr(), hg.data_ptr(), scratch.data_ptr(), need, stream))

    def mm():
        torch.mm(y, w_all.t())
        torch.mm(dl.t(), y)

    cases = {"sweep_step": (lambda: sweep.step(feats, labels, 1.0), steps), "looped_probe_steps": (looped, max(3, steps // G)),
             "sweep_head": (head, steps), "torch_mm_two_gemms": (mm, steps)}
    runs = {k: [] for k in cases}
    for _ in range(repeats):   # alternated windows
        for k, (fn, n) in cases.items():
            runs[k].append(timed(fn, n, min(warmup, n)))
    ms = {k: statistics.median(v) for k, v in runs.items()}
    flop = 4.0 * B * D * G * C
    return {"B": B, "D": D, "C": C, "G": G, "ms": ms, "ms_all": runs, "sweep_launches": SWEEP_LAUNCHES, "looped_launches": SWEEP_LAUNCHES * G,
            "looped_over_sweep": ms["looped_probe_steps"] / ms["sweep_step"], "sweep_step_over_one_probe_step": ms["sweep_step"] / (ms["looped_probe_steps"] / G),
            "gemm_flop": flop, "sweep_head_tflops": flop / (ms["sweep_head"] * 1e-3) / 1e12, "torch_mm_tflops": flop / (ms["torch_mm_two_gemms"] * 1e-3) / 1e12,
            "scratch_mib": need / 2 ** 20}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=60, help="calls per timed window (the looped yardstick makes steps / G, at least 3)")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.set_float32_matmul_precision("highest")
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/probe_sweep_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "cases": [], "notes": []}
    for B, D, C in SHAPES:
        for G in HEADS:
            r = bench(B, D, C, G, args.steps, args.warmup, args.repeats, dev)
            out["cases"].append(r)
            out["notes"].append(f"({B}, {D}, {C}) G = {G}: sweep step {r['ms']['sweep_step'] * 1e3:.1f} us, {G} looped probe steps "
                                f"{r['ms']['looped_probe_steps'] * 1e3:.1f} us (x{r['looped_over_sweep']:.2f}); sweep head {r['ms']['sweep_head'] * 1e3:.1f} us = "
                                f"{r['sweep_head_tflops']:.2f} TFLOP/s, torch.mm {r['ms']['torch_mm_two_gemms'] * 1e3:.1f} us = {r['torch_mm_tflops']:.2f} TFLOP/s")
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
