"""Attentive probing of a frozen encoder on cached patch tokens: one learned query cross-attends over the encoder's tokens, a linear
layer classifies the pooled vector (the frozen-encoder evaluation of V-JEPA and AIM).

The train, validation and test tokens are extracted ONCE (``representation.extract_split_tokens``); every epoch then runs over the
cached tokens, shuffled by a permutation drawn from (seed, epoch) and gathered on the device.  AdamW (weight decay on the three
matrices only, no clipping), cosine learning rate with warm-up, lr = base * batch / 256.  The defaults (lr 1e-3 x batch / 256, weight
decay 0.05, 90 epochs with 10 of warm-up, as many heads as the encoder has) are this tool's own, not a paper's recipe.

    python -m scripts.evaluation.attentive_probe --config configs/ijepa_vits8_attnprobe.yaml --checkpoint outputs/pretrain/ijepa_pretrain/checkpoints/last.ckpt --encoder target
    python -m scripts.evaluation.attentive_probe --config configs/ijepa_vits8_attnprobe.yaml --checkpoint random --synthetic_images 200 --max_epochs 2

Output tree ``outputs/attnprobe/<suffix>/`` (or --output_dir): ``metrics.jsonl`` (one line per epoch: train_loss, train_acc, val_loss,
val_acc, lr, images_per_s), ``attnprobe_last.pt`` (the probe's state: resume with --resume), ``attnprobe_best.pt`` (the state at the
best validation epoch) and ``attnprobe.json`` (val_acc and test_acc at the best validation epoch).  The attentive head has no
classifier-checkpoint format: this tool evaluates its own result.  Every hyper-parameter flag overrides its ``attentive_probe.*``
YAML key.
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

import torch
import yaml

from scripts.evaluation import _probe_cli as C
from scripts.evaluation._probe_cli import epoch_batches, save   # every batch is kept: one image is enough for a step
from ssrl_vit_mae_jepa_amd.attentive import ATTENTIVE_DEFAULTS, TOKEN_SETS, AttentiveProbe, attentive_lr, parse_attentive_probe
from ssrl_vit_mae_jepa_amd.data import STL10_DIR
from ssrl_vit_mae_jepa_amd.training import lr_lambda

HYPER_FLAGS = ("total_epochs", "warmup_epochs", "batch_size", "base_learning_rate", "weight_decay", "heads", "tokens", "bn_eps", "bn_momentum",
               "init_std", "head_init_std")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Attentive probe (one query over cached patch tokens + Linear, AdamW) of a frozen MAE / I-JEPA encoder")
    p.add_argument("--config", type=str, default="configs/ijepa_vits8_attnprobe.yaml")
    p.add_argument("--checkpoint", type=str, required=True, help="checkpoint path (.ckpt / .pt) or 'random'")
    p.add_argument("--encoder", type=str, choices=["target", "context"], default="target", help="I-JEPA encoder (default: the EMA target)")
    p.add_argument("--samples_per_class", type=int, default=None, help="training images per class (default: train.samples_per_class)")
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--max_epochs", type=int, default=None, help="stop after this many epochs (the schedule keeps attentive_probe.total_epochs)")
    p.add_argument("--output_dir_suffix", type=str, default="default")
    p.add_argument("--output_dir", type=str, default=None, help="write here instead of <output_dir_base>/attnprobe/<suffix>")
    p.add_argument("--resume", type=str, default=None, help="an attnprobe_last.pt to continue from")
    for key in HYPER_FLAGS:
        if key == "tokens":
            p.add_argument("--tokens", type=str, choices=list(TOKEN_SETS), default=None, help="patches (default) or all: the class row too, where the encoder has one")
        elif key == "heads":
            p.add_argument("--heads", type=int, default=None, help="overrides attentive_probe.heads (default: the encoder's)")
        else:
            p.add_argument(f"--{key}", type=type(ATTENTIVE_DEFAULTS[key]), default=None, help=f"overrides attentive_probe.{key} (default {ATTENTIVE_DEFAULTS[key]})")
    return p


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def probe_config(cfg: dict, args) -> dict:
    """``attentive_probe:`` of the YAML with every given flag on top, checked; missing keys fall back to ATTENTIVE_DEFAULTS."""
    return parse_attentive_probe(C.merge_flags(cfg.get("attentive_probe"), args, HYPER_FLAGS))


def main(argv=None):
    args = parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    try:
        pcfg = probe_config(cfg, args)
    except ValueError as exc:
        raise SystemExit(f"attentive_probe: {exc}")
    model_cfg = cfg["model"]
    C.check_args("attentive_probe", args, STL10_DIR)
    from ssrl_vit_mae_jepa_amd.representation import extract_split_tokens, load_eval_encoder
    dev = torch.device("cuda", 0)
    seed = int(cfg.get("seed", 73))
    batch = pcfg["batch_size"]

    _, train_b, val_b, test_b = C.labeled_batches(cfg, args, dev)

    precision = cfg.get("engine", {}).get("precision")
    enc = load_eval_encoder(args.checkpoint, model_cfg, encoder=args.encoder, precision=precision, device=dev)
    heads = pcfg["heads"] if pcfg["heads"] is not None else enc.num_heads
    if enc.embed_dim % heads != 0:
        raise SystemExit(f"attentive_probe: heads = {heads} does not divide the encoder width {enc.embed_dim}")
    drop_cls = pcfg["tokens"] == "patches"

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train_t, train_y = extract_split_tokens(enc, train_b, drop_cls=drop_cls)
    val_t, val_y = extract_split_tokens(enc, val_b, drop_cls=drop_cls)
    test_t, test_y = extract_split_tokens(enc, test_b, drop_cls=drop_cls)
    torch.cuda.synchronize()
    extract_s = time.perf_counter() - t0
    n = int(train_y.shape[0])
    if n < 1 or val_t.shape[0] < 1:
        raise SystemExit(f"attentive_probe: {n} training and {val_t.shape[0]} validation images are too few")
    num_classes = int(max(int(train_y.max()), int(val_y.max()), int(test_y.max()))) + 1

    probe = AttentiveProbe(enc.embed_dim, num_classes, heads, pcfg, seed=seed, device=dev)
    start_epoch = 0
    best = dict(val_acc=-1.0, epoch=-1, test_acc=None, test_loss=None)
    if args.resume is not None:
        state = torch.load(args.resume, map_location="cpu", weights_only=False)
        try:
            probe.load_state_dict(state["probe"])
        except ValueError as exc:
            raise SystemExit(f"attentive_probe: --resume: {exc}")
        start_epoch = probe.epoch
        best = dict(state.get("best") or best)   # attnprobe_best.pt is replaced only by a better epoch
    out_dir = Path(args.output_dir) if args.output_dir else Path(cfg.get("logging", {}).get("output_dir_base", "outputs")) / "attnprobe" / args.output_dir_suffix
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "config.yaml").write_text(yaml.safe_dump(dict(cfg, attentive_probe=probe.cfg)))
    peak = attentive_lr(pcfg)
    end_epoch = pcfg["total_epochs"] if args.max_epochs is None else min(pcfg["total_epochs"], start_epoch + args.max_epochs)
    metrics = (out_dir / "metrics.jsonl").open("a" if args.resume else "w")
    for epoch in range(start_epoch, end_epoch):
        lr = peak * lr_lambda(epoch, pcfg["warmup_epochs"], pcfg["total_epochs"])
        loss_sum, correct_sum, rows, dt = C.run_steps(epoch_batches(n, batch, seed, epoch), lambda i, j: (train_t[j], train_y[j]),
                                                      lambda t, y: probe.step(t, y, lr), dev)
        probe.epoch = epoch + 1
        (val_loss,), (val_acc,) = C.evaluate_split(probe, val_t, val_y, batch)
        line = dict(epoch=epoch, train_loss=float(loss_sum) / max(rows, 1), train_acc=int(correct_sum) / max(rows, 1), val_loss=val_loss,
                    val_acc=val_acc, lr=lr, images_per_s=rows / max(dt, 1e-9))
        if val_acc > best["val_acc"]:
            (test_loss,), (test_acc,) = C.evaluate_split(probe, test_t, test_y, batch)
            best = dict(val_acc=val_acc, epoch=epoch, test_acc=test_acc, test_loss=test_loss)
            save(out_dir / "attnprobe_best.pt", dict(probe=probe.state_dict(), best=best, epoch=epoch + 1))
        line["test_acc"] = best["test_acc"]
        metrics.write(json.dumps(line) + "\n")
        metrics.flush()
        print(json.dumps(line))
        save(out_dir / "attnprobe_last.pt", dict(probe=probe.state_dict(), best=best, epoch=epoch + 1))
    metrics.close()
    res = dict(checkpoint=args.checkpoint, kind=enc.kind, encoder=enc.encoder, tokens=pcfg["tokens"], heads=heads, epochs=end_epoch, train_size=n,
               val_size=int(val_t.shape[0]), test_size=int(test_t.shape[0]), tokens_per_image=int(train_t.shape[1]), best_epoch=best["epoch"],
               val_acc=best["val_acc"], test_acc=best["test_acc"], test_loss=best["test_loss"], peak_lr=peak, extract_s=extract_s)
    (out_dir / "attnprobe.json").write_text(json.dumps(res) + "\n")
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
