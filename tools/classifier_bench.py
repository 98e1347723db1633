"""Throughput of the downstream classifier step (images/s), printed as one JSON document.

For each model (the configs/mae.yaml encoder and ViT-S/8 of configs/vits8_dec192.yaml, B = 2000 by default):
  * the native fused step (loss_and_grads + clip + AdamW) with the encoder frozen, unfreeze_last_layers(1) and fully unfrozen;
  * the autograd hand-off (forward_features node + torch Linear head + F.cross_entropy + clip_grad_norm_ + torch AdamW)
    in the last-1 and full modes, alternated with the fused step in the same process;
  * the evaluation forward (no grad).
Device events time `--steps` steps after `--warmup` steps; each number is the median of `--repeats` timed runs.
`--patch_only` runs the encoder over the patch tokens alone (an I-JEPA encoder; no hand-off: forward_features has no such
sequence), `--pool` overrides the config's pool, `--timers` adds the engine's per-kernel-class milliseconds of one fused step.
`--mix` trains with the fine-tuning recipe (mixup 0.8 + CutMix 1.0 + label smoothing 0.1: the batch is mixed on the device every
step and the head takes soft targets) and also times `mae_mix_batch` alone (both kinds of batch, with the bytes it moves);
`--layer_decay X` gives every layer its own learning rate (one AdamW launch per layer instead of one).
`--drop_path X` trains with stochastic depth at rate X: every fused step of an unfrozen mode draws a (2 * depth, B) scale table on
the host, uploads it and runs the scaled LayerNorm kernels (the frozen mode ignores the rate; the hand-off has no drop path and is
not timed then).
`--augment` trains with the per-image augmentation of the recipe in front (RandomResizedCrop(0.08, 1) + flip, rand-m9-mstd0.5-inc1, random
erasing 0.25: a host draw and one `mae_augment_ops_u8` launch per step; no hand-off then) and also times that kernel alone on
draws already on the device -- the crop + flip only (uint8 out) and the whole recipe (fp32 out) -- with the fp64 operations of
their affine ops (counted from the draw: 12 per output pixel for the coordinates, 77 per channel bicubic, 11 bilinear), and the
host's milliseconds per draw.

    python tools/classifier_bench.py --batch 2000 --steps 10 --warmup 3 --out profiles/r04_classifier_bench.json
    python tools/classifier_bench.py --models vits8 --patch_only --pool mean_patches --timers
    python tools/classifier_bench.py --models vits8 --no-handoff --mix --layer_decay 0.75
    python tools/classifier_bench.py --models vits8 --no-handoff --drop_path 0.1
    python tools/classifier_bench.py --models vits8 --no-handoff --augment
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F
import yaml

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae  # noqa: E402


AUGMENT_RECIPE = {"crop_scale": [0.08, 1.0], "flip": 0.5, "interpolation": "bicubic",
                  "rand_augment": {"num_ops": 2, "magnitude": 9.0, "mstd": 0.5, "prob": 0.5}, "random_erasing": 0.25, "fill": 128}


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def set_mode(mod, mode):
    if mode == "frozen":
        mod.freeze_encoder()
    elif mode == "full":
        mod.unfreeze_encoder()
    else:
        mod.unfreeze_last_layers(1)


def bench_model(name: str, cfg_path: Path, B: int, steps: int, warmup: int, repeats: int, modes=("frozen", "last1", "full"),
                handoff: bool = True, patch_only: bool = False, pool=None, timers: bool = False, mix: bool = False,
                layer_decay: float = 1.0, drop_path: float = 0.0, augment: bool = False) -> dict:
    cfg = yaml.safe_load(cfg_path.read_text())
    mc = dict(cfg["model"], general=dict(cfg["model"]["general"], engine_precision=cfg.get("engine", {}).get("precision", "bf16")))
    if pool is not None:
        mc["head"] = dict(mc.get("head") or {}, pool=pool)
    dev = torch.device("cuda", 0)
    mae = encoder_mae(mc)
    mae.encoder.vit.with_cls = not patch_only
    handoff = handoff and not patch_only and mc.get("head", {}).get("pool", "cls") == "cls"  # the hand-off below pools the class token
    handoff = handoff and drop_path == 0.0  # the hand-off has no drop path: not comparable
    handoff = handoff and not augment  # nor per-image augmentation
    recipe = dict(label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0) if mix else {}
    if augment:
        recipe["augment"] = AUGMENT_RECIPE
    mod = ViTClassifierTrainModule(pretrained_encoder=mae.encoder.vit, model_cfg=mc,
                                   training_cfg=dict(cfg.get("train", {}), layer_decay=layer_decay, drop_path=drop_path, **recipe)).to(dev)
    S = mc["general"]["image_size"]
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, 10, (B,), device=dev, generator=g)
    m = mod.model.mae
    ws_bytes = int(mod.model.workspace(B).numel())
    res = {"model": name, "config": str(cfg_path.relative_to(ROOT)), "batch": B, "precision": m.engine.precision,
           "with_cls": not patch_only, "pool": mod.model.pool_type, "workspace_gib": ws_bytes / 2 ** 30, "mix": mix, "layer_decay": layer_decay,
           "drop_path": drop_path, "augment": augment,
           "ms": {}, "images_per_s": {}}

    def fused():
        mod.fused_training_step(images, labels, lr=1e-5)

    def handoff_opt():
        params = [p for p in mod.model.parameters() if p.requires_grad]
        opt = torch.optim.AdamW(params, lr=1e-5, weight_decay=mod.weight_decay)

        def step():
            feats = mod.model.encoder.forward_features(images)
            logits = F.linear(feats[:, 0], mod.model.head.classification.weight, mod.model.head.classification.bias)
            loss = F.cross_entropy(logits, labels)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
            opt.zero_grad(set_to_none=True)
        return step

    def evaluate():
        with torch.no_grad():
            mod.model.evaluate(images, labels, logits=False)

    runs = {}
    for mode in modes:
        set_mode(mod, mode)
        cases = [(f"fused_{mode}", fused)]
        if mode != "frozen" and handoff:
            cases.append((f"handoff_{mode}", handoff_opt()))
        for _r in range(repeats):  # alternated: fused, hand-off, fused, hand-off, ...
            for key, fn in cases:
                runs.setdefault(key, []).append(timed(fn, steps, warmup))
        if timers:  # one more fused step with the engine's event timers on: milliseconds per kernel class
            m.engine.timers_enable(True)
            m.engine.timers_reset()
            fused()
            torch.cuda.synchronize()
            res.setdefault("timers_ms", {})[f"fused_{mode}"] = {k: round(v["ms"], 4) for k, v in m.engine.timers_read().items() if v["launches"]}
            m.engine.timers_enable(False)
    mod.freeze_encoder()
    for _r in range(repeats):
        runs.setdefault("eval_forward", []).append(timed(evaluate, steps, warmup))
    if mix:  # mae_mix_batch alone, parameters already on the device: mixup (uint8 in, fp32 out: 1 + 1 bytes read, 4 written per
        # pixel), CutMix with a half-size box (uint8 -> uint8: 1 read, 1 written) and mixup of an fp32 batch (4 + 4 read, 4 written)
        from ssrl_vit_mae_jepa_amd import _lib
        flip = torch.arange(B - 1, -1, -1, dtype=torch.int32, device=dev)
        lam = torch.full((B,), 0.37, device=dev)
        empty = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        boxes = {"mix_kernel_mixup": empty, "mix_kernel_mixup_fp32": empty,
                 "mix_kernel_cutmix": torch.tensor([[S // 4, 3 * S // 4, S // 4, 3 * S // 4]] * B, dtype=torch.int32, device=dev)}
        f32_out = torch.empty(images.shape, dtype=torch.float32, device=dev)
        srcs = {"mix_kernel_mixup": images, "mix_kernel_mixup_fp32": torch.rand(images.shape, device=dev), "mix_kernel_cutmix": images}
        outs = {"mix_kernel_mixup": f32_out, "mix_kernel_mixup_fp32": f32_out, "mix_kernel_cutmix": torch.empty_like(images)}
        px = images.numel()
        res["mix_kernel_bytes"] = {"mix_kernel_mixup": 6 * px, "mix_kernel_mixup_fp32": 12 * px, "mix_kernel_cutmix": 2 * px}
        stream = torch.cuda.current_stream(dev).cuda_stream

        def raw(key):
            src, out = srcs[key], outs[key]
            dt = lambda t: _lib.MAE_U8 if t.dtype == torch.uint8 else _lib.MAE_F32  # noqa: E731
            return lambda: _lib.check(_lib.lib.mae_mix_batch(src.data_ptr(), dt(src), flip.data_ptr(), lam.data_ptr(), boxes[key].data_ptr(), B,
                                                             images.shape[1], S, dt(out), out.data_ptr(), stream))
        for _r in range(repeats):
            for key in boxes:
                runs.setdefault(key, []).append(timed(raw(key), steps, warmup))
    if augment:  # mae_augment_ops_u8 alone, draws already on the device: the crop + flip (uint8 out), then the whole recipe (fp32 out)
        from ssrl_vit_mae_jepa_amd import _lib
        from ssrl_vit_mae_jepa_amd.classifier import parse_augment
        from ssrl_vit_mae_jepa_amd.data import draw_finetune_augment
        kw = parse_augment(AUGMENT_RECIPE)
        t0 = time.perf_counter()
        for i in range(5):
            full = draw_finetune_augment(B, S, (73, 0, i), **kw)
        res["augment_host_draw_ms"] = (time.perf_counter() - t0) / 5 * 1e3
        draws = {"augment_kernel_crop_flip": draw_finetune_augment(B, S, (73, 0, 0), **dict(kw, num_ops=0, erase_prob=0.0)),
                 "augment_kernel_recipe": full}
        stream = torch.cuda.current_stream(dev).cuda_stream
        res["augment_kernel_fp64_gflop"] = {}

        def raw_aug(p):
            codes, args = p.op_codes.to(dev), p.op_args.to(dev)
            erase = p.erase.to(dev) if p.erase is not None else None
            out = torch.empty(images.shape, dtype=torch.uint8 if erase is None else torch.float32, device=dev)
            return lambda: _lib.check(_lib.lib.mae_augment_ops_u8(images.data_ptr(), B, images.shape[1], S, codes.data_ptr(), args.data_ptr(),
                                                                  codes.shape[1], erase.data_ptr() if erase is not None else None,
                                                                  _lib.MAE_U8 if erase is None else _lib.MAE_F32, out.data_ptr(), stream))
        for key, p in draws.items():
            affine = p.op_codes[:, :, 0] == _lib.AUG_AFFINE
            cubic = affine & ((p.op_codes[:, :, 1] & 1) == 1)
            C = images.shape[1]
            res["augment_kernel_fp64_gflop"][key] = S * S * (int(affine.sum()) * 12 + int(cubic.sum()) * 77 * C + int((affine & ~cubic).sum()) * 11 * C) / 1e9
            fn = raw_aug(p)
            for _r in range(repeats):
                runs.setdefault(key, []).append(timed(fn, steps, warmup))
    for key, v in runs.items():
        ms = statistics.median(v)
        res["ms"][key] = ms
        res["images_per_s"][key] = B / (ms / 1e3)
    res["ms_all"] = runs
    for key, nbytes in res.get("mix_kernel_bytes", {}).items():
        res.setdefault("mix_kernel_gb_per_s", {})[key] = nbytes / (res["ms"][key] * 1e-3) / 1e9
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--models", default="yaml,vits8")
    ap.add_argument("--modes", default="frozen,last1,full")
    ap.add_argument("--no-handoff", action="store_true", help="fused steps only (e.g. under a kernel trace)")
    ap.add_argument("--patch_only", action="store_true", help="the encoder over the patch tokens alone (with_cls = False)")
    ap.add_argument("--pool", choices=["cls", "mean", "mean_patches"], default=None, help="overrides model.head.pool of the config")
    ap.add_argument("--timers", action="store_true", help="per-kernel-class milliseconds of one fused step per mode")
    ap.add_argument("--mix", action="store_true", help="mixup 0.8 + CutMix 1.0 + label smoothing 0.1 in the fused step; times the mix kernel too")
    ap.add_argument("--layer_decay", type=float, default=1.0, help="layer-wise learning-rate decay of the fused step (1 = off)")
    ap.add_argument("--drop_path", type=float, default=0.0, help="stochastic depth rate of the fused step (0 = off)")
    ap.add_argument("--augment", action="store_true", help="crop + flip, RandAugment and random erasing in front of the fused step; times the kernel too")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.backends.cuda.matmul.allow_tf32 = False
    cfgs = {"yaml": ROOT / "configs" / "mae.yaml", "vits8": ROOT / "configs" / "vits8_dec192.yaml"}
    out = {"tool": "tools/classifier_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "results": []}
    for name in args.models.split(","):
        out["results"].append(bench_model(name, cfgs[name], args.batch, args.steps, args.warmup, args.repeats,
                                              tuple(args.modes.split(",")), not args.no_handoff, args.patch_only, args.pool, args.timers, args.mix,
                                              args.layer_decay, args.drop_path, args.augment))
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
