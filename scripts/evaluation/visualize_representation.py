"""2-D projection of frozen-encoder features (the reference's scripts/evaluation/visualize_representation.py) with the
features taken from the engine (``mae_engine_extract_features``) instead of timm ``forward_features`` + host pooling.
Same flags, the same plots (one all-class plot and one class-vs-all plot per class), plus ``--encoder`` (I-JEPA target /
context), ``--synthetic_images``, ``--output_dir`` (default assets/visualizations) and ``--save_features`` (an .npz of the
normalised features and labels).  t-SNE comes from sklearn, the plots from matplotlib; UMAP needs umap-learn.  ``--method tsne_gpu``
is the exact t-SNE of ``ssrl_vit_mae_jepa_amd.embedding.DeviceTSNE`` on the MI355X (PCA initialisation, the same perplexity rule, at
most 16384 samples); it also writes ``<stem>.json`` with the KL trace.  ``--method umap_gpu`` is ``embedding.DeviceUMAP`` (umap-learn's
defaults, exact neighbours, a deterministic layout; at most 16384 samples) and writes ``<stem>.json`` with its parameters.

    python -m scripts.evaluation.visualize_representation --config configs/mae.yaml --encoder_ckpt outputs/pretrain/mae_pretrain/vit-mae.pt --method tsne
"""
from __future__ import annotations

import argparse
import json
from pathlib import Path

import numpy as np
import torch
import yaml

from ssrl_vit_mae_jepa_amd.data import get_test_batches
from ssrl_vit_mae_jepa_amd.representation import apply_normalization, config_depth_dim, extract_split_features, load_eval_encoder, parse_layers

try:
    import umap

    HAS_UMAP = True
except ImportError:
    HAS_UMAP = False

TSNE_GPU_MAX_SAMPLES = 16384  # embedding.MAX_N: what exact t-SNE and UMAP on the device admit
STL10_CLASSES = ["airplane", "bird", "car", "cat", "deer", "dog", "horse", "monkey", "ship", "truck"]


def project(features: np.ndarray, method: str = "umap", seed: int = 73) -> np.ndarray:
    if method == "tsne":
        from sklearn.manifold import TSNE
        print("Running t-SNE...")
        return TSNE(n_components=2, perplexity=min(30.0, max(1.0, (len(features) - 1) / 3)), learning_rate="auto",
                    random_state=seed).fit_transform(features)
    if method == "umap":
        if not HAS_UMAP:
            raise RuntimeError("UMAP requested but not installed.")
        print("Running UMAP...")
        return umap.UMAP(n_components=2).fit_transform(features)
    raise ValueError(f"Unknown method: {method}")


def project_tsne_gpu(features: np.ndarray, device):
    """-> (Z (N, 2) numpy, info): DeviceTSNE from pca_init, perplexity by project()'s rule."""
    from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE
    print("Running t-SNE on the device...")
    tsne = DeviceTSNE(perplexity=min(30.0, max(1.0, (len(features) - 1) / 3)))
    Z, info = tsne.fit(torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(device))
    return Z.cpu().numpy(), info


def project_umap_gpu(features: np.ndarray, device, seed: int = 73):
    """-> (Z (N, 2) numpy, info): DeviceUMAP with umap-learn's defaults from umap_init."""
    from ssrl_vit_mae_jepa_amd.embedding import DeviceUMAP
    print("Running UMAP on the device...")
    Z, info = DeviceUMAP(seed=seed).fit(torch.from_numpy(np.ascontiguousarray(features, dtype=np.float32)).to(device))
    return Z.cpu().numpy(), info


def plot_embedding(Z, y, out_path, title_extra, class_names):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(8, 8))
    for cls in np.unique(y):
        mask = y == cls
        plt.scatter(Z[mask, 0], Z[mask, 1], s=12, label=class_names[cls])
    plt.title(f"2D feature projection ({title_extra})")
    plt.legend(title="Classes", bbox_to_anchor=(1.05, 1), loc="upper left")
    plt.tight_layout()
    plt.savefig(out_path, dpi=300, bbox_inches="tight")
    plt.close()
    print(f"Saved figure to {out_path}")


def plot_class_vs_all(Z, y, class_id, class_name, out_path):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    plt.figure(figsize=(6, 6))
    mask_bg = y != class_id
    plt.scatter(Z[mask_bg, 0], Z[mask_bg, 1], c="lightgray", s=10, label="other")
    mask_cls = y == class_id
    plt.scatter(Z[mask_cls, 0], Z[mask_cls, 1], c="tab:red", s=12, label=class_name)
    plt.title(f"Class {class_name} vs all")
    plt.legend()
    plt.tight_layout()
    plt.savefig(out_path, dpi=300)
    plt.close()


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="2-D projection of frozen encoder features")
    p.add_argument("--config", type=str, default="configs/mae.yaml")
    p.add_argument("--encoder_ckpt", type=str, required=True, help="checkpoint path or 'random'")
    p.add_argument("--method", type=str, choices=["umap", "tsne", "tsne_gpu", "umap_gpu"], default="umap")
    p.add_argument("--pool", type=str, choices=["cls", "mean", "cls_mean"], default="cls", help="cls_mean = [class token | patch mean], with --layers only")
    p.add_argument("--layers", type=str, default=None,
                   help="plot the features after these encoder blocks (last | lastN | each | comma-separated indices; several are concatenated)")
    p.add_argument("--normalize", type=str, choices=["none", "l2", "channel"], default="none")
    p.add_argument("--max_samples", type=int, default=2000)
    p.add_argument("--batch_size", type=int, default=512)
    p.add_argument("--encoder", type=str, choices=["target", "context"], default="target", help="I-JEPA encoder")
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--output_dir", type=str, default=str(Path("assets") / "visualizations"))
    p.add_argument("--save_features", action="store_true", help="also write the normalised features and labels as .npz")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if args.method == "umap" and not HAS_UMAP:
        raise RuntimeError("UMAP requested but not installed.")
    if args.method in ("tsne_gpu", "umap_gpu") and args.max_samples > TSNE_GPU_MAX_SAMPLES:
        raise SystemExit(f"visualize_representation: --method {args.method} embeds at most {TSNE_GPU_MAX_SAMPLES} samples, --max_samples is {args.max_samples}")
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    layers = None
    if args.layers is not None:
        try:
            layers = parse_layers(args.layers, config_depth_dim(cfg["model"])[0])
        except ValueError as exc:
            raise SystemExit(f"visualize_representation: {exc}")
    elif args.pool == "cls_mean":
        raise SystemExit("visualize_representation: --pool cls_mean needs --layers")
    if not torch.cuda.is_available():
        raise SystemExit("visualize_representation: the MI355X engine has no CPU fallback")
    dev = torch.device("cuda", 0)
    enc = load_eval_encoder(args.encoder_ckpt, cfg["model"], encoder=args.encoder, precision=cfg.get("engine", {}).get("precision"), device=dev)
    if not enc.with_cls and args.pool != "mean":
        raise SystemExit("visualize_representation: I-JEPA encoders see no class token: --pool must be mean")
    test_cfg = dict(cfg, test=dict(cfg.get("test", {}), batch_size=args.batch_size))
    batches = get_test_batches(test_cfg, dev, synthetic_images=args.synthetic_images)
    print("Extracting features...")
    feats, labels = extract_split_features(enc, batches, pool=args.pool, normalize="none", max_samples=args.max_samples, layers=layers)
    feats = feats.flatten(1)  # (N, n, W) -> (N, n W) with --layers
    feats = apply_normalization(feats.cpu().numpy(), args.normalize)  # the reference normalises on the host, in numpy
    labels = labels.cpu().numpy()
    print("Projecting to 2D...")
    info = None
    if args.method == "tsne_gpu":
        Z, info = project_tsne_gpu(feats, dev)
    elif args.method == "umap_gpu":
        Z, info = project_umap_gpu(feats, dev)
    else:
        Z = project(feats, method=args.method)
    save_dir = Path(args.output_dir)
    save_dir.mkdir(parents=True, exist_ok=True)
    ckpt_name = "random" if args.encoder_ckpt == "random" else Path(args.encoder_ckpt).parent.parent.stem
    stem = f"representation_{ckpt_name}_{args.method}_{args.pool}_{args.normalize}"
    if enc.kind == "ijepa":
        stem += f"_{enc.encoder}"
    if layers is not None:
        stem += "_blocks" + "-".join(str(l) for l in layers)
    plot_embedding(Z, labels, str(save_dir / f"{stem}.png"), f"{args.method}, pool={args.pool}, norm={args.normalize}", STL10_CLASSES)
    for cls_id in np.unique(labels):
        plot_class_vs_all(Z, labels, cls_id, STL10_CLASSES[cls_id], str(save_dir / f"{stem}_class{cls_id}.png"))
    if args.save_features:
        np.savez(save_dir / f"{stem}.npz", features=feats, labels=labels, projection=Z)
    if info is not None:
        (save_dir / f"{stem}.json").write_text(json.dumps(info, indent=1))
    return save_dir, stem


if __name__ == "__main__":
    main()
