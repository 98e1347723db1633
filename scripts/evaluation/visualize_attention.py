"""Where a frozen encoder looks: per-head attention maps of an encoder block (DINO's class-token maps, or for an encoder without a
class token the attention each patch receives) and attention rollout (Abnar & Zuidema 2020) down to the input patches, from the
engine (``mae_engine_extract_attention``: one forward pass, then column sums of the attention probabilities of the saved qkv).

    python -m scripts.evaluation.visualize_attention --config configs/mae.yaml --checkpoint outputs/pretrain/mae_pretrain/vit-mae.pt --rollout
    python -m scripts.evaluation.visualize_attention --config configs/ijepa_vits8.yaml --checkpoint outputs/pretrain/ijepa_pretrain/checkpoints/last.ckpt --encoder target --layers each
    python -m scripts.evaluation.visualize_attention --config configs/mae.yaml --checkpoint random --synthetic_images 16

Writes <output_dir>/attention_<name>.png -- per image: the input, one heat map per head of the last listed block upsampled to the image,
the head mean and, with --rollout, the rollout -- and <output_dir>/attention.json: per listed block and head the mean entropy of the
map in nats, the mass on the class key, and the entropy ln T of a uniform map for scale.  Prints the JSON's path and one summary line.
"""
from __future__ import annotations

import argparse
import json
import math
from pathlib import Path
from typing import Any, Dict, Optional, Sequence, Tuple

import torch
import yaml

from ssrl_vit_mae_jepa_amd.representation import attention_grid, config_depth_dim, parse_layers

QUERIES = ("cls", "mean")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Attention maps and attention rollout of a frozen MAE / I-JEPA encoder")
    p.add_argument("--config", type=str, default="configs/mae.yaml")
    p.add_argument("--checkpoint", type=str, required=True, help="checkpoint path (.ckpt / .pt) or 'random'")
    p.add_argument("--encoder", type=str, choices=["target", "context"], default="target", help="I-JEPA encoder (default: the EMA target)")
    p.add_argument("--layers", type=str, default="last", help="blocks whose maps are measured: last | lastN | each | comma-separated indices; the figure shows the last one")
    p.add_argument("--query", type=str, choices=QUERIES, default=None, help="cls = the class token's attention (MAE default); mean = the attention each token receives (I-JEPA: the only one)")
    p.add_argument("--rollout", action="store_true", help="also compute attention rollout from the last listed block down to the input")
    p.add_argument("--num_samples", type=int, default=8, help="images in the figure")
    p.add_argument("--batch_size", type=int, default=256)
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--output_dir", type=str, default=str(Path("assets") / "visualizations"))
    return p.parse_args(argv)


def resolve_request(args, model_cfg: Dict[str, Any]) -> Tuple[Tuple[int, ...], str]:
    """(block indices, query) of a command line against the config alone, before anything is loaded; SystemExit on a bad one."""
    depth, _ = config_depth_dim(model_cfg)
    try:
        layers = parse_layers(args.layers, depth)
    except ValueError as exc:
        raise SystemExit(f"visualize_attention: {exc}")
    is_ijepa = "predictor" in model_cfg
    query = args.query or ("mean" if is_ijepa else "cls")
    if query not in QUERIES:
        raise SystemExit(f"visualize_attention: --query must be one of {QUERIES}, got {query!r}")
    if is_ijepa and query != "mean":
        raise SystemExit("visualize_attention: I-JEPA encoders see no class token: --query must be mean")
    if args.num_samples < 1:
        raise SystemExit(f"visualize_attention: --num_samples must be positive, got {args.num_samples}")
    if args.synthetic_images is not None and args.synthetic_images < 1:
        raise SystemExit(f"visualize_attention: --synthetic_images must be positive, got {args.synthetic_images}")
    return layers, query


def attention_stats(maps: torch.Tensor, layers: Sequence[int], with_cls: bool) -> Dict[str, Any]:
    """maps (B, n, H, T) -> per listed block the per-head mean entropy (nats) and mean mass on the class key (0 without one)."""
    B, n, H, T = maps.shape
    if n != len(layers):
        raise ValueError(f"{n} map slices for {len(layers)} blocks")
    p = maps.double()
    ent = -(p * torch.log(p.clamp_min(1e-300))).sum(-1).mean(0)                                  # (n, H)
    cls_mass = p[..., 0].mean(0) if with_cls else torch.zeros(n, H, dtype=torch.float64)         # (n, H)
    return {"tokens": T, "uniform_entropy": math.log(T),
            "blocks": {str(l): {"entropy": [float(v) for v in ent[i]], "class_mass": [float(v) for v in cls_mass[i]]} for i, l in enumerate(layers)}}


def save_attention_figure(images_u8, head_grids, rollout_grid: Optional[Any], path, title: str = "") -> Path:
    """images_u8 (n, C, S, S) uint8, head_grids (n, H, g, g), rollout_grid (n, g, g) or None (torch or numpy): one row per image --
    the input, the H head maps, their mean and the rollout, each map upsampled to the image by nearest neighbour."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    import numpy as np
    imgs = np.asarray(images_u8.cpu() if hasattr(images_u8, "cpu") else images_u8)
    grids = np.asarray(head_grids.cpu() if hasattr(head_grids, "cpu") else head_grids, dtype=np.float64)
    roll = None if rollout_grid is None else np.asarray(rollout_grid.cpu() if hasattr(rollout_grid, "cpu") else rollout_grid, dtype=np.float64)
    if imgs.ndim != 4 or imgs.dtype != np.uint8 or grids.ndim != 4 or grids.shape[0] != imgs.shape[0] or (roll is not None and roll.shape != grids[:, 0].shape):
        raise ValueError(f"expected (n, C, S, S) uint8 images, (n, H, g, g) maps and (n, g, g) rollout, got {imgs.shape} {imgs.dtype}, {grids.shape}, {None if roll is None else roll.shape}")
    n, H, g = grids.shape[0], grids.shape[1], grids.shape[2]
    S = imgs.shape[-1]
    up = max(1, S // g)
    panels = [("input", None)] + [(f"head {h}", grids[:, h]) for h in range(H)] + [("head mean", grids.mean(1))] + ([("rollout", roll)] if roll is not None else [])
    fig, axes = plt.subplots(n, len(panels), figsize=(1.6 * len(panels), 1.7 * n), squeeze=False)
    for r in range(n):
        for c, (name, data) in enumerate(panels):
            ax = axes[r, c]
            if data is None:
                img = imgs[r].transpose(1, 2, 0)
                ax.imshow(img[..., 0] if img.shape[-1] == 1 else img, cmap="gray" if img.shape[-1] == 1 else None, vmin=0, vmax=255)
            else:
                ax.imshow(np.kron(data[r], np.ones((up, up))), cmap="inferno")
            if r == 0:
                ax.set_title(name, fontsize=8)
            ax.axis("off")
    if title:
        fig.suptitle(title, fontsize=9)
    plt.tight_layout()
    path = Path(path)
    path.parent.mkdir(parents=True, exist_ok=True)
    plt.savefig(path, dpi=150, bbox_inches="tight")
    plt.close(fig)
    return path


def main(argv=None):
    args = parse_args(argv)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    layers, query = resolve_request(args, cfg["model"])
    if not torch.cuda.is_available():
        raise SystemExit("visualize_attention: the MI355X engine has no CPU fallback")
    from ssrl_vit_mae_jepa_amd.data import get_test_batches
    from ssrl_vit_mae_jepa_amd.reconstruction import to_display_u8
    from ssrl_vit_mae_jepa_amd.representation import load_eval_encoder
    dev = torch.device("cuda", 0)
    enc = load_eval_encoder(args.checkpoint, cfg["model"], encoder=args.encoder, precision=cfg.get("engine", {}).get("precision"), device=dev)
    if args.query is None:
        query = "cls" if enc.with_cls else "mean"
    if not enc.with_cls and query != "mean":
        raise SystemExit("visualize_attention: this checkpoint holds an encoder without a class token: --query must be mean")
    if enc.depth != config_depth_dim(cfg["model"])[0]:
        raise SystemExit(f"visualize_attention: the encoder has {enc.depth} blocks, the config says {config_depth_dim(cfg['model'])[0]}")
    test_cfg = dict(cfg, test=dict(cfg.get("test", {}), batch_size=args.batch_size))
    batches = get_test_batches(test_cfg, dev, synthetic_images=args.synthetic_images)
    maps, rolls, shown = [], [], None
    for imgs, _ in batches():
        out = enc.attention(imgs, layers=layers, query=query, rollout=args.rollout)
        m, r = out if args.rollout else (out, None)
        maps.append(m.cpu())
        if r is not None:
            rolls.append(r.cpu())
        if shown is None:
            shown = to_display_u8(imgs[:args.num_samples]).cpu()
    if not maps:
        raise SystemExit("visualize_attention: the split holds no image")
    maps = torch.cat(maps)
    roll = torch.cat(rolls) if rolls else None
    stats = attention_stats(maps, layers, enc.with_cls)
    T = maps.shape[-1]
    grid = int(round(math.sqrt(T - (1 if enc.with_cls else 0))))
    n = shown.shape[0]
    name = "random" if args.checkpoint == "random" else Path(args.checkpoint).stem
    stem = f"attention_{name}_{query}" + (f"_{enc.encoder}" if enc.kind == "ijepa" else "") + f"_block{layers[-1]}" + ("_rollout" if args.rollout else "")
    out_dir = Path(args.output_dir)
    fig = save_attention_figure(shown, attention_grid(maps[:n, -1], enc.with_cls, grid), None if roll is None else attention_grid(roll[:n], enc.with_cls, grid),
                                out_dir / f"{stem}.png", f"{name}: block {layers[-1]}, query {query}")
    result = dict(stats, checkpoint=args.checkpoint, kind=enc.kind, encoder=enc.encoder, query=query, layers=list(layers), images=int(maps.shape[0]),
                  heads=int(maps.shape[2]), with_cls=bool(enc.with_cls), figure=str(fig))
    if roll is not None:
        p = roll.double()
        result["rollout"] = {"from_block": int(layers[-1]), "entropy": float(-(p * torch.log(p.clamp_min(1e-300))).sum(-1).mean()),
                             "class_mass": float(p[:, 0].mean()) if enc.with_cls else 0.0}
    (out_dir / "attention.json").write_text(json.dumps(result, indent=2))
    print(f"Saved figure to {fig}")
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
