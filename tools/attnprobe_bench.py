"""Cost of the attentive probe on cached tokens, printed as one JSON document.

Device events, warm-up first, every figure the median of `--repeats` timed windows, at (B, T, D, H) = (2000, 144, 384, 6) and
(256, 256, 1024, 16), ten classes:
  * `mae_attn_pool_fwd` and `mae_attn_pool_bwd` alone, with the bytes/s each achieves on its algorithmic bytes: ONE fp32 read of the
    tokens per pass (4 B T D bytes; what else they touch is H / T of that);
  * one whole `AttentiveProbe.step` (statistics: two more reads of the tokens; the small products; the head; AdamW);
  * in the same process, the copy-rate yardstick of tools/hbm_stream_reference.py (its method: torch's device copy and sum on a buffer
    of the tokens' size, the median of 7 single calls), and each pool kernel's rate as a fraction of the read rate (`sum`).

    python tools/attnprobe_bench.py --out profiles/r26_attnprobe_bench.json
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
from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe  # noqa: E402

SHAPES = [(2000, 144, 384, 6), (256, 256, 1024, 16)]
CLASSES = 10
# statistics (two column sums with their second stages, the finish), fold, pool forward, project, the head (rows, reduce, weight gradient, its
# second stage, a copy), project backward (two products, a second stage, the scale), pool backward with its second stage, fold backward, AdamW x 3
STEP_LAUNCHES = 5 + 1 + 1 + 1 + 5 + 4 + 2 + 1 + 3


def median_ms(fn, steps, warmup, repeats):
    runs = [timed(fn, steps, warmup) for _ in range(repeats)]
    return statistics.median(runs), runs


def yardstick(nbytes: int, dev) -> dict:
    """tools/hbm_stream_reference.py's copy (read + write) and sum (read) on a buffer of nbytes: TB/s, the median of 7 single calls."""
    n = nbytes // 4
    x = torch.rand(n, device=dev)
    y = torch.empty_like(x)
    out = {}
    for fn, name, factor in ((lambda: y.copy_(x), "copy", 2), (lambda: x.sum(), "sum", 1)):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(7):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        out[name + "_tb_per_s"] = factor * n * 4 / (sorted(ts)[3] * 1e-3) / 1e12
    return out


def bench_shape(B, T, D, H, steps, warmup, repeats, dev) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    tokens = torch.randn(B, T, D, device=dev, generator=g) * 1.5 + 0.5
    labels = torch.randint(0, CLASSES, (B,), device=dev, generator=g)
    probe = AttentiveProbe(D, CLASSES, H, device=dev)
    probe.step(tokens, labels, 1e-3)          # fills probe.last: the statistics, uq, ybar and lse the kernels are timed with
    L = {k: v.clone() for k, v in probe.last.items()}
    lib, ptr = _lib.lib, lambda t: t.data_ptr() if t is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    ybar, lse = torch.empty_like(L["ybar"]), torch.empty_like(L["lse"])
    gbuf = torch.randn(B, H, D, device=dev, generator=g) * 1e-3
    duq = torch.empty(H, D, device=dev)
    need = lib.mae_attn_pool_bwd_scratch_bytes(B, T, D, H)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    nbytes = 4 * B * T * D
    cases = {
        "pool_fwd": (lambda: _lib.check(lib.mae_attn_pool_fwd(ptr(tokens), ptr(L["mean"]), ptr(L["uq"]), B, T, D, H, ptr(ybar), ptr(lse), stream)), nbytes),
        "pool_bwd": (lambda: _lib.check(lib.mae_attn_pool_bwd(ptr(tokens), ptr(L["mean"]), ptr(L["uq"]), ptr(L["lse"]), ptr(L["ybar"]), ptr(gbuf), B, T, D, H,
                                                              ptr(duq), ptr(scratch), need, stream)), nbytes),
        "step": (lambda: probe.step(tokens, labels, 1e-3), None),
    }
    res = {"B": B, "T": T, "D": D, "H": H, "token_bytes": nbytes, "ms": {}, "ms_all": {}, "tb_per_s": {}, "fraction_of_sum_rate": {}}
    res["yardstick"] = yardstick(nbytes, dev)
    for key, (fn, nb) in cases.items():
        ms, runs = median_ms(fn, steps, warmup, repeats)
        res["ms"][key], res["ms_all"][key] = ms, runs
        if nb is not None:
            res["tb_per_s"][key] = nb / (ms * 1e-3) / 1e12
            res["fraction_of_sum_rate"][key] = res["tb_per_s"][key] / res["yardstick"]["sum_tb_per_s"]
    res["step_launches"] = STEP_LAUNCHES
    res["step_token_reads"] = 4   # two for the statistics, one per pool pass
    res["step_tb_per_s_on_4_reads"] = 4 * nbytes / (res["ms"]["step"] * 1e-3) / 1e12
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=20, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/attnprobe_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "shapes": []}
    for B, T, D, H in SHAPES:
        out["shapes"].append(bench_shape(B, T, D, H, args.steps, args.warmup, args.repeats, dev))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
