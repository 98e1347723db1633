"""Supervised fine-tuning / linear probing of the classifier on the MI355X engine (the reference's
scripts/training/train_mae.py, without Lightning): same flags, YAML keys and output tree
``outputs/train/<suffix>/{checkpoints/{best,last}.ckpt, logs/metrics.jsonl, config.yaml, <logging.model_path>}``.

    python -m scripts.training.train_mae --config configs/mae.yaml --encoder_ckpt outputs/pretrain/mae_pretrain/checkpoints/last.ckpt

Model branches as the reference (:85-161): --classifier_ckpt (weights only, fresh optimizer), --encoder_ckpt (encoder
weights found by prefix), or the random-init baseline.  --encoder_ckpt also takes an I-JEPA checkpoint (detected by its
layout): --encoder picks the EMA target (default) or the context encoder, the classifier then runs over the patch tokens
alone and pools with mean_patches unless model.head.pool / --pool says otherwise (cls is refused: no class token).

    python -m scripts.training.train_mae --config configs/ijepa_vits8.yaml --encoder_ckpt outputs/pretrain/ijepa_pretrain/checkpoints/last.ckpt  Freeze precedence (:167-176): train.unfreeze_last_layers, then
train.freeze_encoder.  Each epoch: the native fused step over the training split, a no-grad validation pass, the
per-epoch LR, one metrics line; best.ckpt on a new maximum of val_acc, last.ckpt every epoch.

The fine-tuning recipe of the MAE paper: --label_smoothing, --mixup, --cutmix and --layer_decay override the YAML keys
train.label_smoothing / mixup_alpha / cutmix_alpha / layer_decay (configs/vits8_dec192_finetune.yaml sets 0.1, 0.8, 1.0, 0.75);
--drop_path overrides train.drop_path (stochastic depth, default 0; the MAE recipe uses 0.1; ignored by a frozen encoder).
--augment turns on the per-image augmentation in front of the mixing (train.augment: RandomResizedCrop + flip, RandAugment
rand-m9-mstd0.5-inc1, random erasing 0.25; configs/vits8_dec192_finetune_aug.yaml); --crop_scale LO HI, --rand_augment N M and
--random_erasing P override its keys.  Training batches only: validation and test images are never augmented.  A model of
another size than the 96 px dataset (model.general.image_size) gets its batches resized on the device; with train.augment the ops run
on the dataset's own pixels first (the kernel holds an image in LDS), then the resize, then the mixing at the model's size.
Under mixup / CutMix the metrics line's ``train_loss`` is the soft-target loss and ``train_acc`` counts argmax == the image's
own label (the first of each mixed pair), so it reads lower than the accuracy on clean images; ``val_*`` stay hard-label.

    python -m scripts.training.train_mae --config configs/vits8_dec192_finetune.yaml --encoder_ckpt outputs/pretrain/mae_pretrain/checkpoints/last.ckpt

--accumulate_grad_batches N overrides train.accumulate_grad_batches: N micro-batches of train.batch_size feed one optimizer
step (the MAE fine-tuning recipe's batch of 1024 on a smaller memory budget); train.learning_rate stays absolute, the mixing,
drop-path and augmentation draws stay per micro-batch, and --max_steps_per_epoch counts optimizer steps.
"""
from __future__ import annotations

import argparse
import json
import os
import time
from pathlib import Path

import torch
import yaml

from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, checkpoint_with_cls, encoder_mae, load_encoder_weights
from ssrl_vit_mae_jepa_amd.data import accumulation_plan, accumulation_slots, get_train_batches
from ssrl_vit_mae_jepa_amd.representation import checkpoint_layout, load_ijepa_encoder

SEED = 73
PREFIXES = ("model.encoder.", "encoder.", "module.encoder.")
IJEPA_LAYOUTS = ("ijepa_ckpt", "ijepa_pt")
NO_CLS = "train_mae: I-JEPA encoders see no class token: --pool must be mean or mean_patches"


AUGMENT_RECIPE = {"crop_scale": [0.08, 1.0], "flip": 0.5, "interpolation": "bicubic",
                  "rand_augment": {"num_ops": 2, "magnitude": 9.0, "mstd": 0.5, "prob": 0.5}, "random_erasing": 0.25, "fill": 128}


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description="Fine-tune / linear-probe the ViT classifier")
    parser.add_argument("--config", type=str, default="configs/mae.yaml")
    parser.add_argument("--encoder_ckpt", type=str, default=None, help="Path to a pretrained MAE or I-JEPA checkpoint (encoder weights)")
    parser.add_argument("--classifier_ckpt", type=str, default=None, help="Path to a full classifier checkpoint")
    parser.add_argument("--output_dir_suffix", type=str, default="mae_finetune", help="Suffix for the output directory")
    # additions (not in the reference): I-JEPA encoders and the pool override; bounded runs
    parser.add_argument("--encoder", type=str, choices=["target", "context"], default="target",
                        help="which I-JEPA encoder to fine-tune (ignored for MAE checkpoints)")
    parser.add_argument("--pool", type=str, choices=["cls", "mean", "mean_patches"], default=None, help="overrides model.head.pool")
    # the fine-tuning recipe (not in the reference): each overrides its train.* key
    parser.add_argument("--label_smoothing", type=float, default=None, help="overrides train.label_smoothing (eps of the soft target)")
    parser.add_argument("--mixup", type=float, default=None, help="overrides train.mixup_alpha (0 = off)")
    parser.add_argument("--cutmix", type=float, default=None, help="overrides train.cutmix_alpha (0 = off)")
    parser.add_argument("--layer_decay", type=float, default=None, help="overrides train.layer_decay (1 = one learning rate)")
    parser.add_argument("--drop_path", type=float, default=None, help="overrides train.drop_path (stochastic depth rate, 0 = off)")
    parser.add_argument("--augment", action="store_true",
                        help="per-image augmentation with the recipe's defaults: RandomResizedCrop(0.08, 1) + flip, rand-m9-mstd0.5-inc1, random erasing 0.25")
    parser.add_argument("--crop_scale", type=float, nargs=2, default=None, metavar=("LO", "HI"), help="overrides train.augment.crop_scale")
    parser.add_argument("--rand_augment", type=float, nargs=2, default=None, metavar=("N", "M"),
                        help="overrides train.augment.rand_augment.num_ops / magnitude")
    parser.add_argument("--random_erasing", type=float, default=None, help="overrides train.augment.random_erasing (probability, 0 = off)")
    parser.add_argument("--accumulate_grad_batches", type=int, default=None,
                        help="micro-batches per optimizer step (overrides train.accumulate_grad_batches, default 1)")
    parser.add_argument("--max_epochs", type=int, default=None)
    parser.add_argument("--max_steps_per_epoch", type=int, default=None)
    parser.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    return parser


def parse_args(argv=None):
    return build_parser().parse_args(argv)


def augment_overrides(args, block):
    """train.augment after --augment / --crop_scale / --rand_augment / --random_erasing: --augment fills in the recipe's defaults
    under what the YAML sets, each other flag overrides its key; None when neither the YAML nor a flag asks for augmentation."""
    import copy
    block = copy.deepcopy(block) if block else {}
    if getattr(args, "augment", False):
        merged = copy.deepcopy(AUGMENT_RECIPE)
        ra = dict(merged["rand_augment"], **(block.get("rand_augment") or {}))
        merged.update(block)
        merged["rand_augment"] = ra
        block = merged
    if getattr(args, "crop_scale", None) is not None:
        block["crop_scale"] = [float(v) for v in args.crop_scale]
    if getattr(args, "rand_augment", None) is not None:
        block["rand_augment"] = dict(block.get("rand_augment") or {}, num_ops=int(args.rand_augment[0]), magnitude=float(args.rand_augment[1]))
    if getattr(args, "random_erasing", None) is not None:
        block["random_erasing"] = float(args.random_erasing)
    return block or None


def apply_recipe_flags(cfg: dict, args) -> None:
    """--label_smoothing / --mixup / --cutmix / --layer_decay / --drop_path / --accumulate_grad_batches into cfg["train"]; a flag that was not given changes nothing."""
    for flag, key in (("label_smoothing", "label_smoothing"), ("mixup", "mixup_alpha"), ("cutmix", "cutmix_alpha"), ("layer_decay", "layer_decay"),
                      ("drop_path", "drop_path")):
        if getattr(args, flag, None) is not None:
            cfg["train"][key] = float(getattr(args, flag))
    if getattr(args, "accumulate_grad_batches", None) is not None:
        cfg["train"]["accumulate_grad_batches"] = int(args.accumulate_grad_batches)
    block = augment_overrides(args, cfg["train"].get("augment"))
    if block is not None:
        cfg["train"]["augment"] = block


def model_config(cfg: dict) -> dict:
    m = cfg["model"]
    return dict(m, general=dict(m["general"], engine_precision=cfg.get("engine", {}).get("precision", "bf16")))


def load_state(path: str) -> dict:
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    return ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt


def is_ijepa_state(state: dict) -> bool:
    try:
        return checkpoint_layout(state) in IJEPA_LAYOUTS
    except ValueError:
        return False


def resolve_pool(model_cfg: dict, pool=None, ijepa: bool = False) -> dict:
    """model_cfg with the pool the run uses: --pool, else model.head.pool, else mean_patches for an I-JEPA encoder (cls for
    everything else, the reference's default).  cls on an I-JEPA encoder ends the run."""
    head = dict(model_cfg.get("head") or {})
    if pool is not None:
        head["pool"] = pool
    elif ijepa and "pool" not in head:
        head["pool"] = "mean_patches"
    if ijepa and head.get("pool", "cls") == "cls":
        raise SystemExit(NO_CLS)
    return dict(model_cfg, head=head)


def build_module(cfg: dict, encoder_ckpt=None, classifier_ckpt=None, encoder: str = "target", pool=None) -> ViTClassifierTrainModule:
    model_cfg, train_cfg = model_config(cfg), cfg["train"]
    if classifier_ckpt:
        print(f"Loading full classifier checkpoint: {classifier_ckpt}")
        ckpt = torch.load(classifier_ckpt, map_location="cpu", weights_only=True)
        state = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
        vit = encoder_mae(model_cfg).encoder.vit
        vit.with_cls = checkpoint_with_cls(ckpt)  # a classifier fine-tuned from I-JEPA stays on the patch tokens alone
        hp = (ckpt.get("hyper_parameters") or {}) if isinstance(ckpt, dict) else {}
        if pool is None and "with_cls" in hp:  # such a checkpoint carries the pool its head was trained with
            pool = ((hp.get("model_cfg") or {}).get("head") or {}).get("pool")
        model_cfg = resolve_pool(model_cfg, pool, ijepa=not vit.with_cls)
        module = ViTClassifierTrainModule(pretrained_encoder=vit, model_cfg=model_cfg, training_cfg=train_cfg)
        if not any(k.startswith("model.") for k in state):
            state = {"model." + k: v for k, v in state.items()}  # a bare module.model.state_dict() (.pt)
        module.load_state_dict(state, strict=False)
    elif encoder_ckpt:
        print(f"Loading pretrained encoder: {encoder_ckpt}")
        state = load_state(encoder_ckpt)
        if is_ijepa_state(state):
            model_cfg = resolve_pool(model_cfg, pool, ijepa=True)
            vit = load_ijepa_encoder(state, model_cfg, encoder=encoder)
            print(f"Loaded the I-JEPA {encoder} encoder (patch tokens only, pool {model_cfg['head']['pool']})")
        else:
            model_cfg = resolve_pool(model_cfg, pool)
            mae = encoder_mae(model_cfg)
            if not any(k.startswith(p) for p in PREFIXES for k in state):
                raise ValueError("Could not find encoder weights in checkpoint. Expected keys starting with one of: " + ", ".join(PREFIXES))
            missing, unexpected = load_encoder_weights(mae, state)
            print(f"Loaded encoder weights ({len(missing)} missing, {len(unexpected)} unexpected)")
            vit = mae.encoder.vit
        module = ViTClassifierTrainModule(pretrained_encoder=vit, model_cfg=model_cfg, training_cfg=train_cfg)
    else:
        print("Baseline: random-initialized VisionTransformer (no MAE)")
        module = ViTClassifierTrainModule(pretrained_encoder=None, model_cfg=resolve_pool(model_cfg, pool), training_cfg=train_cfg)
    if train_cfg.get("unfreeze_last_layers", None) is not None:
        module.unfreeze_last_layers(int(train_cfg["unfreeze_last_layers"]))
    elif train_cfg.get("freeze_encoder", True):
        module.freeze_encoder()
    else:
        module.unfreeze_encoder()
    return module


def save(path: Path, obj) -> None:
    tmp = path.with_suffix(path.suffix + ".tmp")
    torch.save(obj, tmp)
    os.replace(tmp, path)


def main(argv=None):
    args = parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    apply_recipe_flags(cfg, args)
    if not torch.cuda.is_available():
        raise SystemExit("train_mae: the MI355X engine has no CPU fallback")
    dev = torch.device("cuda", 0)
    torch.manual_seed(SEED)
    train_cfg, log_cfg = cfg["train"], cfg["logging"]
    output_dir = Path(log_cfg["output_dir_base"]) / "train" / args.output_dir_suffix
    ckpt_dir = output_dir / "checkpoints"
    ckpt_dir.mkdir(parents=True, exist_ok=True)
    (output_dir / "logs").mkdir(exist_ok=True)
    with open(output_dir / "config.yaml", "w") as f_out:
        yaml.safe_dump(cfg, f_out)

    # train.augment runs on the dataset's own pixels and the module resizes afterwards: its training batches leave the loader as stored
    train_batches, val_batches = get_train_batches(cfg, dev, synthetic_images=args.synthetic_images, seed=SEED,
                                                   train_at_dataset_size=bool(train_cfg.get("augment")))
    module = build_module(cfg, args.encoder_ckpt, args.classifier_ckpt, encoder=args.encoder, pool=args.pool).to(dev)
    module.mix_seed = module.drop_seed = module.aug_seed = int(cfg.get("seed", SEED))  # the mixup / CutMix, drop-path and augmentation draws of a step are functions of (seed, epoch, step)
    total = int(train_cfg["total_epochs"]) if args.max_epochs is None else min(int(train_cfg["total_epochs"]), args.max_epochs)
    best_acc, log_path = -1.0, output_dir / "logs" / "metrics.jsonl"
    for epoch in range(total):
        module.current_epoch = epoch
        lr = module.current_lr(epoch)
        t0, seen = time.perf_counter(), 0
        sums = torch.zeros(2, dtype=torch.float64, device=dev)  # [sum of batch-mean loss * rows, correct]
        plan = accumulation_plan(train_batches.n, train_batches.batch, module.accumulate_grad_batches)
        slots = accumulation_slots(plan if args.max_steps_per_epoch is None else plan[:args.max_steps_per_epoch])
        for (index, count, window_rows, _before), (imgs, labels) in zip(slots, train_batches(epoch)):
            loss, correct = module.fused_training_step(imgs, labels, lr=lr, accumulate=(index, count), window_rows=window_rows)
            if index == count - 1:  # the window's mean loss and its correct count
                sums[0] += loss[0].double() * window_rows
                sums[1] += correct[0].double()
                seen += window_rows
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        val = torch.zeros(2, dtype=torch.float64, device=dev)
        n_val = 0
        with torch.no_grad():
            for imgs, labels in val_batches():
                _l, loss, correct = module.model.evaluate(imgs, labels, logits=False)
                val[0] += loss[0].double() * imgs.shape[0]
                val[1] += correct[0].double()
                n_val += imgs.shape[0]
        rec = dict(epoch=epoch, train_loss=float(sums[0]) / max(1, seen), train_acc=float(sums[1]) / max(1, seen),
                   val_loss=float(val[0]) / max(1, n_val), val_acc=float(val[1]) / max(1, n_val), lr=lr, images_per_s=seen / dt)
        with open(log_path, "a") as f:
            f.write(json.dumps(rec) + "\n")
        print(json.dumps(rec))
        ckpt = module.checkpoint(epoch)
        ckpt["val_acc"] = rec["val_acc"]
        if rec["val_acc"] > best_acc:
            best_acc = rec["val_acc"]
            save(ckpt_dir / "best.ckpt", ckpt)
        save(ckpt_dir / "last.ckpt", ckpt)
    model_path = output_dir / log_cfg["model_path"]
    torch.save({k: v.detach().cpu() for k, v in module.model.state_dict().items()}, model_path)
    print(f"Training complete; model weights saved to: {model_path}; best checkpoint: {ckpt_dir / 'best.ckpt'}")


if __name__ == "__main__":
    main()
