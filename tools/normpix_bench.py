"""Cost of normalised-pixel targets (norm_pix_loss) on the bench workload, printed as one JSON document.

ViT-S/8 96 px (configs/vits8_dec192.yaml), batch 2000, bf16, uint8 and fp32 images.  Two modules with the same weights, one
with the flag and one without (the yardstick: the plain masked-pixel MSE kernels), live in the same process and are timed
alternately:
  * the whole fused step (loss_and_grads + clip + AdamW), device events around `--steps` steps after `--warmup`, no kernel
    timers; median of `--repeats` alternated runs;
  * the engine's `mse_loss` timer class (Engine.timers_read) over `--steps` instrumented steps, ms per launch.

    python tools/normpix_bench.py --out profiles/r10_normpix_bench.json
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

from ssrl_vit_mae_jepa_amd import MAEPretrainModule  # noqa: E402


def build(cfg: dict, flag: bool, batch: int, dev) -> MAEPretrainModule:
    general = dict(cfg["model"]["general"], engine_precision="bf16")
    if flag:
        general["norm_pix_loss"] = True
    torch.manual_seed(73)
    module = MAEPretrainModule(dict(general=general, encoder=cfg["model"]["encoder"], decoder=cfg["model"]["decoder"]),
                               dict(cfg["pretrain"], batch_size=batch)).to(dev)
    module.on_train_epoch_start()
    return module


def timed_steps(module, images, noises, steps: int, warmup: int) -> float:
    for i in range(warmup):
        module.fused_training_step(images, noises[i])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for i in range(steps):
        module.fused_training_step(images, noises[warmup + i])
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def loss_class_ms(module, images, noises, steps: int) -> dict:
    eng = module.model.engine
    eng.timers_reset()
    eng.timers_enable(True)
    for i in range(steps):
        module.fused_training_step(images, noises[i])
    torch.cuda.synchronize()
    eng.timers_enable(False)
    t = eng.timers_read()["mse_loss"]
    return dict(ms_per_launch=t["ms"] / max(1, t["launches"]), launches=t["launches"], bytes_per_launch=t["bytes"] / max(1, t["launches"]))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=str(ROOT / "configs" / "vits8_dec192.yaml"))
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("normpix_bench: the MI355X engine has no CPU fallback")
    dev = torch.device("cuda", 0)
    cfg = yaml.safe_load(open(args.config))
    general = cfg["model"]["general"]
    S, chans, L = int(general["image_size"]), int(general.get("in_chans", 3)), (int(general["image_size"]) // int(general["patch_size"])) ** 2 + 1
    modules = {"off": build(cfg, False, args.batch, dev), "on": build(cfg, True, args.batch, dev)}
    g = torch.Generator(device=dev).manual_seed(73)
    u8 = torch.randint(0, 256, (args.batch, chans, S, S), device=dev, generator=g, dtype=torch.uint8)
    inputs = {"uint8": u8, "fp32": (u8.float() / 255.0 - 0.5) / 0.5}
    noises = [torch.rand(args.batch, L, device=dev, generator=g) for _ in range(args.warmup + args.steps)]
    res = dict(workload=f"{Path(args.config).name}, batch {args.batch}, bf16", steps=args.steps, warmup=args.warmup, repeats=args.repeats, rows={})
    for name, images in inputs.items():
        runs = {"off": [], "on": []}
        for _r in range(args.repeats):
            for flag, module in modules.items():
                runs[flag].append(timed_steps(module, images, noises, args.steps, args.warmup))
        row = {}
        for flag, module in modules.items():
            row[flag] = dict(step_ms=statistics.median(runs[flag]), step_ms_runs=runs[flag], mse_loss=loss_class_ms(module, images, noises, args.steps))
        row["mse_loss_ratio"] = row["on"]["mse_loss"]["ms_per_launch"] / row["off"]["mse_loss"]["ms_per_launch"]
        row["step_ratio"] = row["on"]["step_ms"] / row["off"]["step_ms"]
        res["rows"][name] = row
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
