"""Cost of the linear probe on cached features, printed as one JSON document.

Device events, warm-up first, every figure the median of `--repeats` timed windows:
  * one `LinearProbe.step` at (B, D, C) = (2000, 384, 10) and (16384, 1024, 100);
  * each kernel of the step alone at those shapes -- `mae_batchnorm_fwd` in training and evaluation mode, `mae_lars_step` with and
    without the trust ratio -- with the bytes/s it achieves on its algorithmic bytes (BatchNorm training: x read three times, y
    written once = 16 B per element; evaluation 8 B; LARS with the norms 28 B per element: p and g for the norms, p, g, mu read and
    p, mu written by the update; without them 20 B);
  * one probe epoch over 5000 cached ViT-S/8 features (the permutation, the gathers and three steps at batch 2000), and the one-off
    extraction of those features;
  * the frozen-encoder step and the evaluation forward of tools/classifier_bench.py at batch 2000, in the same process: what an
    epoch of probing costs per batch when the features are not cached.

    python tools/probe_bench.py --out profiles/r07_probe_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from classifier_bench import bench_model, timed  # noqa: E402
from scripts.evaluation.linear_probe import epoch_batches  # noqa: E402
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.probe import LinearProbe, probe_lr  # noqa: E402

SHAPES = [(2000, 384, 10), (16384, 1024, 100)]
# BatchNorm (two column sums with their second stages, the sweep), the head (rows, reduce, weight gradient, its second stage, a copy), LARS on
# W (norms, finalize, update), LARS on b
STEP_LAUNCHES = 5 + 5 + 3 + 1


def median_ms(fn, steps, warmup, repeats):
    runs = [timed(fn, steps, warmup) for _ in range(repeats)]
    return statistics.median(runs), runs


def bench_shape(B, D, C, steps, warmup, repeats, dev) -> dict:
    g = torch.Generator(device=dev).manual_seed(0)
    feats = torch.randn(B, D, device=dev, generator=g) * 2 + 3
    labels = torch.randint(0, C, (B,), device=dev, generator=g)
    probe = LinearProbe(D, C, device=dev)
    lr = probe_lr(probe.cfg)
    res = {"B": B, "D": D, "C": C, "ms": {}, "ms_all": {}, "bytes": {}, "gb_per_s": {}}
    lib, ptr = _lib.lib, lambda t: t.data_ptr() if t is not None else None
    stream = torch.cuda.current_stream(dev).cuda_stream
    y = torch.empty_like(feats)
    rm, rv = torch.zeros(D, device=dev), torch.ones(D, device=dev)
    need = lib.mae_batchnorm_scratch_bytes(B, D)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    n = C * D
    p, gr, mu = torch.randn(n, device=dev) * 0.01, torch.randn(n, device=dev) * 1e-3, torch.zeros(n, device=dev)
    ls = torch.empty(4096, device=dev)
    cases = {
        "step": (lambda: probe.step(feats, labels, lr), None),
        "batchnorm_train": (lambda: _lib.check(lib.mae_batchnorm_fwd(ptr(feats), B, D, 1e-6, 1, 0.1, ptr(rm), ptr(rv), ptr(y), None, None, ptr(scratch),
                                                                     need, stream)), 16 * B * D),
        "batchnorm_eval": (lambda: _lib.check(lib.mae_batchnorm_fwd(ptr(feats), B, D, 1e-6, 0, 0.1, ptr(rm), ptr(rv), ptr(y), None, None, None, 0, stream)),
                           8 * B * D),
        "lars_adapt": (lambda: _lib.check(lib.mae_lars_step(ptr(p), ptr(gr), ptr(mu), n, 1, 1e-3, 0.9, 0.0, 0.001, None, ptr(ls), stream)), 28 * n),
        "lars_plain": (lambda: _lib.check(lib.mae_lars_step(ptr(p), ptr(gr), ptr(mu), n, 0, 1e-3, 0.9, 0.0, 0.001, None, ptr(ls), stream)), 20 * n),
    }
    for key, (fn, nbytes) in cases.items():
        ms, runs = median_ms(fn, steps, warmup, repeats)
        res["ms"][key], res["ms_all"][key] = ms, runs
        if nbytes is not None:
            res["bytes"][key] = nbytes
            res["gb_per_s"][key] = nbytes / (ms * 1e-3) / 1e9
    res["step_launches"] = STEP_LAUNCHES
    res["step_us_per_launch"] = res["ms"]["step"] * 1e3 / STEP_LAUNCHES
    return res


def bench_epoch(n, batch, steps, warmup, repeats, dev) -> dict:
    from ssrl_vit_mae_jepa_amd.data import synthetic_labeled
    from ssrl_vit_mae_jepa_amd.representation import load_eval_encoder
    cfg = yaml.safe_load((ROOT / "configs" / "vits8_dec192_linprobe.yaml").read_text())
    enc = load_eval_encoder("random", cfg["model"], precision=cfg["engine"]["precision"], device=dev)
    imgs, labels = synthetic_labeled(n)
    imgs, labels = imgs.to(dev), torch.from_numpy(labels).to(dev)

    def extract():
        return torch.cat([enc.features(imgs[i:i + 500], pool="cls", normalize="none") for i in range(0, n, 500)])
    extract_ms, extract_runs = median_ms(extract, 1, 1, repeats)
    feats = extract()
    probe = LinearProbe(feats.shape[1], 10, dict(batch_size=batch), device=dev)
    lr = probe_lr(probe.cfg)
    state = {"epoch": 0}

    def epoch():
        for idx in epoch_batches(n, batch, 73, state["epoch"]):
            j = torch.from_numpy(idx).to(dev)
            probe.step(feats[j], labels[j], lr)
        state["epoch"] += 1
    ms, runs = median_ms(epoch, steps, warmup, repeats)
    nsteps = len(epoch_batches(n, batch, 73, 0))
    return {"images": n, "batch": batch, "dim": int(feats.shape[1]), "steps_per_epoch": nsteps, "epoch_ms": ms, "epoch_ms_all": runs,
            "extract_ms": extract_ms, "extract_ms_all": extract_runs, "images_per_s_cached_epoch": n / (ms * 1e-3)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200, help="probe steps / kernel calls / epochs per timed window")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--encoder_steps", type=int, default=10, help="steps per timed window of the frozen-encoder step")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.backends.cuda.matmul.allow_tf32 = False
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/probe_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "shapes": [], "notes": []}
    for B, D, C in SHAPES:
        out["shapes"].append(bench_shape(B, D, C, args.steps, args.warmup, args.repeats, dev))
    out["epoch"] = bench_epoch(5000, 2000, max(1, args.steps // 4), max(1, args.warmup // 4), args.repeats, dev)
    torch.cuda.empty_cache()
    enc = bench_model("vits8", ROOT / "configs" / "vits8_dec192.yaml", 2000, args.encoder_steps, 3, args.repeats, modes=("frozen",), handoff=False)
    out["frozen_encoder_step"] = {"batch": 2000, "ms": enc["ms"], "ms_all": enc["ms_all"]}
    ep, fr = out["epoch"], enc["ms"]["fused_frozen"]
    uncached = fr * 5000 / 2000
    out["epoch"]["frozen_encoder_epoch_ms"] = uncached
    out["epoch"]["cached_over_frozen"] = ep["epoch_ms"] / uncached
    small = out["shapes"][0]
    kernels = sum(small["ms"][k] for k in ("batchnorm_train", "lars_adapt", "lars_plain"))
    out["notes"].append(f"a step at {SHAPES[0]} takes {small['ms']['step'] * 1e3:.1f} us over {STEP_LAUNCHES} launches "
                        f"({small['step_us_per_launch']:.1f} us per launch); its BatchNorm and LARS calls alone take {kernels * 1e3:.1f} us")
    out["notes"].append(f"a cached epoch of 5000 features takes {ep['epoch_ms']:.3f} ms against {uncached:.1f} ms of frozen-encoder steps for the same images "
                        f"(x{uncached / ep['epoch_ms']:.0f}); extracting the 5000 features once takes {ep['extract_ms']:.1f} ms")
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
