"""What a pretrained MAE reconstructs (the reference's scripts/evaluation/visualize_reconstruction.py): the 3 x n figure
"Original / Masked / Reconstructed" of the first training images and the MSE / L1 / PSNR block, with the forward, the image
composition and the error sums taken from the engine (``mae_engine_reconstruct``).  Same flags (--config, --model_path,
--output_path_suffix), plus --model_path random (the chance baseline), --synthetic_images, --num_samples, --mask_seed,
--batch_size, --norm_pix_loss (weights trained against normalised-pixel targets, for checkpoints that do not record it),
--output_dir (default assets/visualizations) and --eval_split val (the same statistics over the whole
validation split).  Writes the PNG and ``reconstruction_stats.json`` next to it.

    python -m scripts.evaluation.visualize_reconstruction --config configs/mae.yaml --model_path outputs/pretrain/mae_pretrain/checkpoints/last.ckpt
    python -m scripts.evaluation.visualize_reconstruction --config configs/mae.yaml --model_path outputs/pretrain/mae_pretrain/vit-mae.pt --eval_split val
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import torch
import yaml

from ssrl_vit_mae_jepa_amd.data import STL10_DIR, _load_stl10_labeled, get_train_batches
from ssrl_vit_mae_jepa_amd.reconstruction import MASK_SEED, MAEReconstructor, evaluate_reconstruction


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Reconstruct image")
    p.add_argument("--config", type=str, default="configs/mae.yaml", help="Path to the YAML config file.")
    p.add_argument("--model_path", type=str, default="outputs/pretrain/mae_100/checkpoints/best.ckpt",
                   help="Path to the model checkpoint, or 'random'.")
    p.add_argument("--output_path_suffix", type=str, default="reconstruction_validation.png", help="Suffix to append to the output path.")
    # additions (not in the reference)
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--num_samples", type=int, default=8, help="images in the figure")
    p.add_argument("--mask_seed", type=int, default=MASK_SEED)
    p.add_argument("--batch_size", type=int, default=None, help="default: train.batch_size of the config")
    p.add_argument("--output_dir", type=str, default=str(Path("assets") / "visualizations"))
    p.add_argument("--eval_split", type=str, choices=["none", "val"], default="none", help="val: also the statistics of the whole validation split")
    p.add_argument("--norm_pix_loss", action="store_true",
                   help="the weights were trained against normalised-pixel targets (for a bare state dict such as vit-mae.pt, which "
                        "records no flag; a Lightning checkpoint carries its own)")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.num_samples < 1:
        raise SystemExit("visualize_reconstruction: --num_samples must be >= 1")
    with open(args.config, "r") as f:
        config = yaml.safe_load(f)
    if not torch.cuda.is_available():
        raise SystemExit("visualize_reconstruction: the MI355X engine has no CPU fallback")
    if args.synthetic_images is None and _load_stl10_labeled("train") is None:  # a synthetic stand-in is never used silently
        raise SystemExit(f"visualize_reconstruction: the labeled STL-10 files ({STL10_DIR}/train_*.bin) are missing; "
                         "pass --synthetic_images N to run on synthetic images")
    dev = torch.device("cuda", 0)
    train_cfg = dict(config.get("train", {}))
    train_cfg["batch_size"] = max(args.num_samples, int(args.batch_size or train_cfg.get("batch_size", 64)))
    train_batches, val_batches = get_train_batches(dict(config, train=train_cfg), dev, synthetic_images=args.synthetic_images)
    if train_batches.n < args.num_samples:
        raise SystemExit(f"visualize_reconstruction: the train split holds {train_batches.n} images, --num_samples asks for {args.num_samples}")

    model_cfg = config["model"]
    mask_ratio = config.get("pretrain", {}).get("mask_ratio_end", 0.75)
    reconstructor = MAEReconstructor(model_path=args.model_path, device=str(dev), mask_ratio=mask_ratio, mask_seed=args.mask_seed,
                                     precision=config.get("engine", {}).get("precision"))
    general_cfg = dict(model_cfg["general"], norm_pix_loss=True) if args.norm_pix_loss else model_cfg["general"]
    reconstructor.load_model(general_cfg, model_cfg["encoder"], model_cfg["decoder"])
    if reconstructor.model.norm_pix_loss:
        print("norm_pix_loss: the model predicts standardised patches; images and statistics are de-normalised (pixel space)")

    save_dir = Path(args.output_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    png = save_dir / args.output_path_suffix
    sample = reconstructor.validate_reconstruction(dataloader=train_batches, num_samples=args.num_samples, save_path=str(png))
    res = dict(model_path=args.model_path, layout=reconstructor.layout, data="stl10" if args.synthetic_images is None else "synthetic",
               mask_ratio=mask_ratio, mask_seed=args.mask_seed, norm_pix_loss=reconstructor.model.norm_pix_loss, figure=str(png), sample=sample)
    if args.eval_split == "val":
        res["val"] = evaluate_reconstruction(reconstructor.model, val_batches, mask_ratio=mask_ratio, mask_seed=args.mask_seed)
        print(f"\nValidation split ({res['val']['images']} images): MSE {res['val']['mse']:.6f}, MAE {res['val']['l1']:.6f}, "
              f"PSNR {res['val']['psnr']:.2f} dB, masked-patch MSE {res['val']['masked_mse']:.6f}")
    (png.parent / "reconstruction_stats.json").write_text(json.dumps(res, indent=1) + "\n")
    return res


if __name__ == "__main__":
    main()
