"""Linear probing of a frozen encoder on cached features: the protocol of the MAE paper (A.1, Table 10) and of I-JEPA --
BatchNorm1d(affine=False) + Linear trained with LARS (no weight decay, momentum 0.9, no clipping), lr = base * batch / 256.

The train, validation and test features are extracted ONCE (``representation.extract_split_features``); every epoch then runs
over the cached features (shuffled by a permutation drawn from (seed, epoch), batches gathered on the device), so a 90-epoch
probe pays one encoder pass instead of ninety.  ``--augment crop`` re-extracts the training features every step from
RandomResizedCrop + flip images (``data.augment_to_size``: the box is drawn on the stored image and resampled straight to the
model's size, parameters drawn from (seed, epoch, step)); validation and test features stay cached.

    python -m scripts.evaluation.linear_probe --config configs/vits8_dec192_linprobe.yaml --checkpoint outputs/pretrain/mae_pretrain/checkpoints/last.ckpt
    python -m scripts.evaluation.linear_probe --config configs/ijepa_vits8.yaml --checkpoint outputs/pretrain/ijepa_pretrain/checkpoints/last.ckpt --encoder target
    python -m scripts.evaluation.evaluate_classifier --config configs/vits8_dec192_linprobe.yaml --checkpoint outputs/probe/linprobe/checkpoints/best.ckpt

Output tree ``outputs/probe/<suffix>/``: ``logs/metrics.jsonl`` (one line per epoch: train_loss, train_acc, val_loss, val_acc, lr,
images_per_s), ``checkpoints/{best,last}.ckpt`` (classifier checkpoints with BatchNorm folded into the head, read by
``train_mae.build_module(classifier_ckpt=...)`` and ``evaluate_classifier`` unchanged), ``checkpoints/probe_last.pt`` (the probe's own
state: resume with --resume) and ``probe.json`` (test_acc / test_loss at the best validation epoch).  Every hyper-parameter flag
overrides its ``probe.*`` YAML key.

``--sweep_lr 0.01,0.03,0.1,0.3,1.0 --sweep_wd 0,0.0005`` (or the top-level YAML block ``probe_sweep: {base_learning_rate: [...],
weight_decay: [...]}``; a flag overrides its key, a missing axis takes the single ``probe.*`` value, at most 64 heads) trains the
whole grid of heads in ONE pass (``probe.ProbeSweep``): the features of a step are formed once and shared, every head follows the same
epochs and schedule shape at its own peak learning rate, and the head with the best validation accuracy wins (ties: the lower
validation loss, then the lower index).  ``logs/metrics.jsonl`` then holds per-head lists, ``sweep.json`` one row per head (lr, wd, best
validation accuracy, its epoch, test accuracy / loss at that epoch) and the winner's index, ``probe.json`` the winner's figures plus
``sweep_index``, ``best.ckpt`` the winner at its best epoch, ``last.ckpt`` the current leader and ``probe_last.pt`` the whole sweep
(``--resume`` refuses a state whose grid differs).

``--layers SPEC`` (last | lastN | each | 2,5,-1) probes the concatenated features of those encoder blocks, each through the encoder's final
LayerNorm (DINO's and I-JEPA's last-n-blocks probe), from one forward pass per batch; ``--pool cls_mean`` then gives [class token |
patch mean] per block.  The concatenation must fit the probe kernels' 1024 columns (ViT-S: two blocks).  Such a head reads no single
encoder output, so no classifier checkpoint is written: ``probe_last.pt`` and ``probe.json`` carry ``layers`` instead.
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

import numpy as np
import torch
import yaml

from scripts.evaluation import _probe_cli as C
from scripts.evaluation._probe_cli import EXTRACT_BATCH, save
from ssrl_vit_mae_jepa_amd.data import STL10_DIR, augment_to_size, draw_augment_params, labeled_serving
from ssrl_vit_mae_jepa_amd.probe import (AUGMENTS, PROBE_DEFAULTS, LinearProbe, ProbeSweep, classifier_pool, parse_probe, parse_sweep, probe_lr,
                                         select)
from ssrl_vit_mae_jepa_amd.training import lr_lambda

HYPER_FLAGS = ("total_epochs", "warmup_epochs", "batch_size", "base_learning_rate", "weight_decay", "momentum", "trust_coefficient", "bn_eps",
               "bn_momentum", "head_init_std", "augment")
PROBE_MAX_DIM = 1024  # columns the probe kernels take (probe.ProbeHead)


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Linear probe (BatchNorm + Linear, LARS) of a frozen MAE / I-JEPA encoder on cached features")
    p.add_argument("--config", type=str, default="configs/vits8_dec192_linprobe.yaml")
    p.add_argument("--checkpoint", type=str, required=True, help="checkpoint path (.ckpt / .pt) or 'random'")
    p.add_argument("--encoder", type=str, choices=["target", "context"], default="target", help="I-JEPA encoder (default: the EMA target)")
    p.add_argument("--pool", type=str, choices=["cls", "mean", "mean_all", "cls_mean"], default=None,
                   help="feature pool; MAE default cls, I-JEPA mean; cls_mean = [class token | patch mean], with --layers only")
    p.add_argument("--layers", type=str, default=None,
                   help="probe the concatenated features of these encoder blocks: last | lastN | each | comma-separated indices")
    p.add_argument("--samples_per_class", type=int, default=None, help="training images per class (default: train.samples_per_class)")
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--max_epochs", type=int, default=None, help="stop after this many epochs (the schedule keeps probe.total_epochs)")
    p.add_argument("--output_dir_suffix", type=str, default="linprobe")
    p.add_argument("--resume", type=str, default=None, help="a probe_last.pt to continue from")
    p.add_argument("--sweep_lr", type=str, default=None,
                   help="comma-separated base learning rates: train one head per (lr, wd) pair in one pass (overrides probe_sweep.base_learning_rate)")
    p.add_argument("--sweep_wd", type=str, default=None, help="comma-separated weight decays of the sweep (overrides probe_sweep.weight_decay)")
    for key in HYPER_FLAGS:
        kind = type(PROBE_DEFAULTS[key])
        if key == "augment":
            p.add_argument("--augment", type=str, choices=list(AUGMENTS), default=None, help="overrides probe.augment")
        else:
            p.add_argument(f"--{key}", type=kind, default=None, help=f"overrides probe.{key} (default {PROBE_DEFAULTS[key]})")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def probe_config(cfg: dict, args) -> dict:
    """``probe:`` of the YAML with every given flag on top, checked."""
    return parse_probe(C.merge_flags(cfg.get("probe"), args, HYPER_FLAGS))


def epoch_batches(n: int, batch: int, seed: int, epoch: int):
    """Index arrays of the epoch's batches; the last partial batch is used only if it has at least 2 rows (BatchNorm needs two)."""
    return C.epoch_batches(n, batch, seed, epoch, min_rows=2)


def _features(enc, images: torch.Tensor, pool: str, layers=None) -> torch.Tensor:
    return torch.cat([enc.features(images[i:i + EXTRACT_BATCH], pool=pool, normalize="none", layers=layers).flatten(1)
                      for i in range(0, images.shape[0], EXTRACT_BATCH)])


def probe_layers(spec, model_cfg: dict, pool: str):
    """(layers, feature width) of --layers SPEC, or (None, embed_dim) without it; SystemExit when the spec is wrong or the concatenation
    is wider than the probe kernels take.  Needs the config alone: it runs before any data or checkpoint is loaded."""
    from ssrl_vit_mae_jepa_amd.representation import config_depth_dim, parse_layers
    depth, dim = config_depth_dim(model_cfg)
    if spec is None:
        if pool == "cls_mean":
            raise SystemExit("linear_probe: --pool cls_mean needs --layers")
        return None, dim
    try:
        layers = parse_layers(spec, depth)
    except ValueError as exc:
        raise SystemExit(f"linear_probe: {exc}")
    width = len(layers) * dim * (2 if pool == "cls_mean" else 1)
    if width > PROBE_MAX_DIM:
        raise SystemExit(f"linear_probe: --layers {spec} with pool {pool} gives {width} feature columns ({len(layers)} blocks x "
                         f"{width // len(layers)}); the probe kernels take at most {PROBE_MAX_DIM}")
    return layers, width


def main(argv=None):
    args = parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    try:
        pcfg = probe_config(cfg, args)
        grid = parse_sweep(cfg.get("probe_sweep"), pcfg, args.sweep_lr, args.sweep_wd)   # None: no sweep asked for
    except ValueError as exc:
        raise SystemExit(f"linear_probe: {exc}")
    model_cfg = cfg["model"]
    is_ijepa = "predictor" in model_cfg
    pool = args.pool or ("mean" if is_ijepa else "cls")
    if is_ijepa and pool in ("cls", "cls_mean"):
        raise SystemExit("linear_probe: I-JEPA encoders see no class token: --pool must be mean or mean_all")
    layers, width = probe_layers(args.layers, model_cfg, pool)   # before any data or checkpoint is loaded
    C.check_args("linear_probe", args, STL10_DIR)
    from ssrl_vit_mae_jepa_amd.representation import extract_split_features, load_eval_encoder
    dev = torch.device("cuda", 0)
    seed = int(cfg.get("seed", 73))
    batch = pcfg["batch_size"]
    data_cfg, train_b, val_b, test_b = C.labeled_batches(cfg, args, dev)

    precision = cfg.get("engine", {}).get("precision")
    enc = load_eval_encoder(args.checkpoint, model_cfg, encoder=args.encoder, precision=precision, device=dev)
    try:
        classifier_pool("cls" if pool == "cls_mean" else pool, enc.with_cls)   # cls_mean follows the rule of cls: it needs the class token
    except ValueError as exc:
        raise SystemExit(f"linear_probe: {exc}")

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    crop = pcfg["augment"] == "crop"
    crop_size, crop_dtype = labeled_serving(data_cfg)   # the model's size: the crop is resampled straight to it (None: the stored size)
    if crop:   # the training features are re-extracted per step: only the images and labels are kept, at the stored resolution
        train_images, train_f, train_y = train_b.images[train_b.idx], None, train_b.labels[train_b.idx]
    else:
        train_images, (train_f, train_y) = None, extract_split_features(enc, train_b, pool=pool, normalize="none", layers=layers)
        train_f = train_f.flatten(1)   # (N, n, W) -> (N, n W) with --layers
    val_f, val_y = extract_split_features(enc, val_b, pool=pool, normalize="none", layers=layers)
    test_f, test_y = extract_split_features(enc, test_b, pool=pool, normalize="none", layers=layers)
    val_f, test_f = val_f.flatten(1), test_f.flatten(1)
    torch.cuda.synchronize()
    extract_s = time.perf_counter() - t0
    n = int(train_y.shape[0])
    if n < 2 or val_f.shape[0] < 1:
        raise SystemExit(f"linear_probe: {n} training and {val_f.shape[0]} validation rows are too few")
    num_classes = int(max(int(train_y.max()), int(val_y.max()), int(test_y.max()))) + 1

    # One loop for the probe and the sweep, on per-head lists throughout (a single probe is one head).  The two differ in the object
    # built, in what step() is handed, in the resume refusals and in what is written: lists and the sweep's extra keys with a grid,
    # scalars without.
    sweep = grid is not None
    heads = [dict(pcfg, **g) for g in grid] if sweep else [pcfg]   # every head's hyper-parameters
    G, peaks = len(heads), [probe_lr(h) for h in heads]
    dim = enc.embed_dim if layers is None else width
    probe = ProbeSweep(dim, num_classes, grid, pcfg, seed=seed, device=dev) if sweep else LinearProbe(dim, num_classes, pcfg, seed=seed, device=dev)
    written = (lambda v: v) if sweep else (lambda v: v[0])
    start_epoch = 0
    best = [dict(val_acc=-1.0, val_loss=None, epoch=-1, test_acc=None, test_loss=None) for _ in range(G)]
    if args.resume is not None:
        state = torch.load(args.resume, map_location="cpu", weights_only=False)
        if sweep and "grid" not in state:
            raise SystemExit(f"linear_probe: --resume {args.resume} holds a single probe, this run asks for a sweep of {G} heads")
        if not sweep and "grid" in state:
            raise SystemExit(f"linear_probe: --resume {args.resume} holds a sweep of {len(state['grid'])} heads; pass its grid (--sweep_lr / --sweep_wd)")
        if list(state.get("layers") or []) != list(layers or []) or (layers is not None and state.get("pool") != pool):
            raise SystemExit(f"linear_probe: --resume state was trained on layers {state.get('layers')} pool {state.get('pool')}, "
                             f"this run asks for layers {None if layers is None else list(layers)} pool {pool}")
        try:
            probe.load_state_dict(state)
        except ValueError as exc:
            raise SystemExit(f"linear_probe: --resume: {exc}")
        start_epoch = probe.epoch
        best = [dict(b) for b in state["best"]] if sweep else [dict(state.get("best") or best[0])]   # best.ckpt is replaced only by a better epoch
    out_dir = Path(cfg.get("logging", {}).get("output_dir_base", "outputs")) / "probe" / args.output_dir_suffix
    (out_dir / "checkpoints").mkdir(parents=True, exist_ok=True)
    (out_dir / "logs").mkdir(parents=True, exist_ok=True)
    axes = {k: list(dict.fromkeys(g[k] for g in grid)) for k in ("base_learning_rate", "weight_decay")} if sweep else None
    (out_dir / "config.yaml").write_text(yaml.safe_dump(dict(cfg, probe=pcfg, probe_sweep=axes) if sweep else dict(cfg, probe=pcfg)))
    end_epoch = pcfg["total_epochs"] if args.max_epochs is None else min(pcfg["total_epochs"], start_epoch + args.max_epochs)
    winner = lambda: select([b["val_acc"] for b in best], [float("inf") if b.get("val_loss") is None else b["val_loss"] for b in best])
    as_probe = lambda g: probe.export(g) if sweep else probe   # head g as a LinearProbe, for its classifier checkpoint
    written_best = lambda: best if sweep else {k: v for k, v in best[0].items() if k != "val_loss"}   # the single probe's entry has no val_loss
    metrics = (out_dir / "logs" / "metrics.jsonl").open("a" if args.resume else "w")
    for epoch in range(start_epoch, end_epoch):
        factor = lr_lambda(epoch, pcfg["warmup_epochs"], pcfg["total_epochs"])
        lr = factor if sweep else peaks[0] * factor   # ProbeSweep.step scales every head's own peak itself; LinearProbe.step takes the rate

        def gather(step, j):   # the batch's features: cached, or re-extracted from a fresh crop of its images
            if not crop:
                return train_f[j], train_y[j]
            imgs = train_images[j].contiguous()
            g = torch.Generator().manual_seed(int(np.random.SeedSequence([seed, epoch, step]).generate_state(1)[0]))
            return _features(enc, augment_to_size(imgs, crop_size, draw_augment_params(imgs.shape[0], imgs.shape[2], g), crop_dtype), pool, layers), train_y[j]

        loss_sum, correct_sum, rows, dt = C.run_steps(epoch_batches(n, batch, seed, epoch), gather, lambda f, y: probe.step(f, y, lr), dev)
        probe.epoch = epoch + 1
        val_loss, val_acc = C.evaluate_split(probe, val_f, val_y, batch)
        leader = select(val_acc, val_loss)   # this epoch's
        line = dict(epoch=epoch, train_loss=written([v / max(rows, 1) for v in loss_sum.tolist()]),
                    train_acc=written([v / max(rows, 1) for v in correct_sum.tolist()]), val_loss=written(val_loss), val_acc=written(val_acc),
                    lr=[float(x) for x in probe.head_lrs(factor)] if sweep else lr)
        if sweep:
            line["leader"] = leader
        line["images_per_s"] = rows / max(dt, 1e-9)
        metrics.write(json.dumps(line) + "\n")
        metrics.flush()
        print(json.dumps(line))
        improved = [g for g in range(G) if val_acc[g] > best[g]["val_acc"]]
        if improved:   # the test split is evaluated whenever a head improves
            test_loss, test_acc = C.evaluate_split(probe, test_f, test_y, batch)
            for g in improved:
                best[g] = dict(val_acc=val_acc[g], val_loss=val_loss[g], epoch=epoch, test_acc=test_acc[g], test_loss=test_loss[g])
        if layers is None:   # a head on several blocks is no classifier head (the classifier reads the last block alone): no classifier checkpoint then
            ckpt = as_probe(leader).classifier_checkpoint(enc, model_cfg, pool, epoch=epoch)
            save(out_dir / "checkpoints" / "last.ckpt", ckpt)
            w = winner()
            if w in improved:   # the winner's entry is of this epoch (an entry changes only by improving, so no other head can take over)
                save(out_dir / "checkpoints" / "best.ckpt", ckpt if w == leader else as_probe(w).classifier_checkpoint(enc, model_cfg, pool, epoch=epoch))
        extra = {} if layers is None else dict(layers=list(layers), pool=pool)
        save(out_dir / "checkpoints" / "probe_last.pt", dict(probe.state_dict(), best=written_best(), **extra))
    metrics.close()
    w = winner()
    res = dict(checkpoint=args.checkpoint, kind=enc.kind, encoder=enc.encoder, pool=pool,
               classifier_pool=classifier_pool(pool, enc.with_cls) if layers is None else None,
               augment=pcfg["augment"], epochs=end_epoch, train_size=n, val_size=int(val_f.shape[0]), test_size=int(test_f.shape[0]),
               best_epoch=best[w]["epoch"], val_acc=best[w]["val_acc"], test_acc=best[w]["test_acc"], test_loss=best[w]["test_loss"],
               peak_lr=peaks[w], extract_s=extract_s)
    if sweep:
        table = [dict(index=g, base_learning_rate=grid[g]["base_learning_rate"], weight_decay=grid[g]["weight_decay"], peak_lr=peaks[g],
                      best_val_acc=best[g]["val_acc"], best_val_loss=best[g]["val_loss"], best_epoch=best[g]["epoch"], test_acc=best[g]["test_acc"],
                      test_loss=best[g]["test_loss"]) for g in range(G)]
        (out_dir / "sweep.json").write_text(json.dumps(dict(winner=w, heads=table)) + "\n")
        res.update(sweep_index=w, sweep_heads=G, base_learning_rate=grid[w]["base_learning_rate"], weight_decay=grid[w]["weight_decay"])
    if layers is not None:
        res["layers"] = list(layers)
    (out_dir / "probe.json").write_text(json.dumps(res) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
