"""Cost of gradient accumulation, printed as one JSON document.

Device events, warm-up first, the variants alternating inside one run, every figure the median of `--repeats` timed windows:
  * ViT-S/8 96 px bf16 (configs/vits8_dec192.yaml): one optimizer step on 2000 images against one window of 4 micro-batches of 500
    images (the same 2000 images and noise, `accumulate=(i, 4)`), both as images/s;
  * `mae_engine_grad_accumulate` alone over that model's trainable range (+ the loss slot's 4 floats), accumulating and overwriting,
    with the bytes/s it achieves on its algorithmic bytes (12 B per element: dst read, src read, dst written; 8 B with overwrite)
    against the 6.29 TB/s copy rate of the MI355X.  A window of A micro-batches runs the sweep A times (A - 1 into the stash, one
    back into the live gradients).

    python tools/accum_bench.py --out profiles/r17_accum_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ssrl_vit_mae_jepa_amd import MAEPretrainModule, _lib  # noqa: E402

COPY_TBPS = 6.29  # measured copy rate of the MI355X's HBM (read + write)


def timed(fn, steps: int) -> float:
    """Milliseconds per call over `steps` calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def alternate(cases: dict, steps: int, warmup: int, repeats: int) -> dict:
    for fn in cases.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            runs[k].append(timed(fn, steps))
    return {k: {"ms": statistics.median(v), "ms_all": v} for k, v in runs.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", default=str(ROOT / "configs" / "vits8_dec192.yaml"))
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--accumulate", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="optimizer steps per timed window")
    ap.add_argument("--kernel_steps", type=int, default=200, help="kernel calls per timed window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.batch % args.accumulate:
        raise SystemExit("--batch must divide by --accumulate")
    dev = torch.device("cuda", 0)
    cfg = yaml.safe_load(Path(args.config).read_text())
    precision = cfg.get("engine", {}).get("precision", "bf16")
    mcfg = dict(cfg["model"], general=dict(cfg["model"]["general"], engine_precision=precision))
    module = MAEPretrainModule(mcfg, dict(cfg["pretrain"], batch_size=args.batch // args.accumulate, accumulate_grad_batches=args.accumulate)).to(dev)
    module.on_train_epoch_start()
    model = module.model
    B, A, micro = args.batch, args.accumulate, args.batch // args.accumulate
    g = torch.Generator(device=dev).manual_seed(73)
    size = model.image_size
    images = torch.rand(B, model.in_chans, size, size, device=dev, generator=g) * 2 - 1
    noise = torch.rand(B, model.sequence_length, device=dev, generator=g)
    parts = [(images[i:i + micro].contiguous(), noise[i:i + micro].contiguous()) for i in range(0, B, micro)]

    def one_step():
        module.fused_training_step(images, noise)

    def one_window():
        for i, (x, z) in enumerate(parts):
            module.fused_training_step(x, z, global_rows=B, accumulate=(i, A))

    out = {"tool": "tools/accum_bench.py", "steps": args.steps, "kernel_steps": args.kernel_steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "config": Path(args.config).name,
           "precision": precision, "batch": B, "accumulate": A, "micro_batch": micro, "notes": []}
    steps = alternate({"step": one_step, "window": one_window}, args.steps, args.warmup, args.repeats)
    for k, v in steps.items():
        v["images_per_s"] = B / (v["ms"] * 1e-3)
    out["step_vs_window"] = steps
    out["step_vs_window"]["window_over_step"] = steps["window"]["ms"] / steps["step"]["ms"]

    n = model.engine.trainable_elems + 4
    live, stash = model.grad_buffer, module._stash()
    h, stream = model.engine.handle, torch.cuda.current_stream(dev).cuda_stream

    def kernel(overwrite):
        return lambda: _lib.check(_lib.lib.mae_engine_grad_accumulate(h, stash.data_ptr(), live.data_ptr(), 0, n, overwrite, stream))

    kern = alternate({"accumulate": kernel(0), "overwrite": kernel(1)}, args.kernel_steps, 20, args.repeats)
    for k, per in (("accumulate", 12), ("overwrite", 8)):
        kern[k]["bytes"] = per * n
        kern[k]["tb_per_s"] = per * n / (kern[k]["ms"] * 1e-3) / 1e12
        kern[k]["share_of_copy_rate"] = kern[k]["tb_per_s"] / COPY_TBPS
    out["kernel"] = dict(kern, elements=n, copy_rate_tb_per_s=COPY_TBPS)
    sweeps_ms = kern["overwrite"]["ms"] + (A - 1) * kern["accumulate"]["ms"]
    out["notes"].append(f"one step of {B} images takes {steps['step']['ms']:.2f} ms, one window of {A} x {micro} {steps['window']['ms']:.2f} ms "
                        f"(x{out['step_vs_window']['window_over_step']:.3f}); the window's {A} accumulate sweeps over {n} elements take {sweeps_ms:.3f} ms of it")
    out["notes"].append(f"the accumulate sweep moves {12 * n / 1e6:.1f} MB in {kern['accumulate']['ms'] * 1e3:.1f} us: {kern['accumulate']['tb_per_s']:.2f} TB/s, "
                        f"{100 * kern['accumulate']['share_of_copy_rate']:.0f} % of the {COPY_TBPS} TB/s copy rate (memory-bound: no arithmetic to speak of)")
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
