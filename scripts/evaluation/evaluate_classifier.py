"""Test-split accuracy of a trained classifier on the MI355X engine (the reference's
scripts/evaluation/evaluate_classifier.py): ``--checkpoint`` defaults to
``outputs/train/<train.output_dir_suffix or "default">/checkpoints/best.ckpt``; a Lightning-shaped ``.ckpt`` or the
``.pt`` state_dict the fine-tuning CLI writes.  A ``.ckpt`` of a classifier fine-tuned from an I-JEPA encoder carries
``with_cls: False`` and its pool, so it is evaluated over the patch tokens alone without further flags.  Prints test_acc / test_loss and writes ``outputs/test/<suffix>/metrics.json``.

    python -m scripts.evaluation.evaluate_classifier --config configs/mae.yaml --checkpoint outputs/train/mae_finetune/checkpoints/best.ckpt
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import torch
import yaml

from scripts.training.train_mae import build_module
from ssrl_vit_mae_jepa_amd.data import get_test_batches


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description="Evaluate a trained ViT classifier on the test split")
    parser.add_argument("--config", type=str, default="configs/mae.yaml")
    parser.add_argument("--checkpoint", type=str, default=None, help="Path to checkpoint (.ckpt or .pt)")
    parser.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    return parser.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    if not torch.cuda.is_available():
        raise SystemExit("evaluate_classifier: the MI355X engine has no CPU fallback")
    dev = torch.device("cuda", 0)
    log_cfg, train_cfg = cfg["logging"], cfg.get("train", {})
    suffix = train_cfg.get("output_dir_suffix", "default")
    if args.checkpoint is None:
        args.checkpoint = str(Path(log_cfg["output_dir_base"]) / "train" / suffix / "checkpoints" / "best.ckpt")
        print(f"Using default checkpoint: {args.checkpoint}")
    module = build_module(cfg, classifier_ckpt=args.checkpoint).to(dev)
    tot = torch.zeros(2, dtype=torch.float64, device=dev)
    n = 0
    with torch.no_grad():
        for imgs, labels in get_test_batches(cfg, dev, synthetic_images=args.synthetic_images)():
            _l, loss, correct = module.model.evaluate(imgs, labels, logits=False)
            tot[0] += loss[0].double() * imgs.shape[0]
            tot[1] += correct[0].double()
            n += imgs.shape[0]
    res = dict(test_acc=float(tot[1]) / max(1, n), test_loss=float(tot[0]) / max(1, n), images=n, checkpoint=args.checkpoint)
    out = Path(log_cfg["output_dir_base"]) / "test" / suffix
    out.mkdir(parents=True, exist_ok=True)
    with open(out / "metrics.json", "w") as f:
        json.dump(res, f, indent=2)
    print(f"test_acc: {res['test_acc']:.4f}")
    print(f"test_loss: {res['test_loss']:.4f}")


if __name__ == "__main__":
    main()
