"""Weighted k-NN accuracy of a frozen encoder (DINO-style probe: l2-normalised features, cosine similarity, exp(sim / T)
votes).  The bank is the labeled STL-10 train split (all 5000 images, or the per-class subset fine-tuning uses with
--samples_per_class); the queries are the test split.  One top-k search at max k, one vote per k, all on the MI355X.
Prints one JSON line and writes it to <output_dir>/knn.json.

    python -m scripts.evaluation.knn_eval --config configs/mae.yaml --checkpoint outputs/pretrain/mae_pretrain/vit-mae.pt
    python -m scripts.evaluation.knn_eval --config configs/ijepa_vits8.yaml --checkpoint outputs/pretrain/ijepa_pretrain/checkpoints/last.ckpt --encoder target
    python -m scripts.evaluation.knn_eval --config configs/mae.yaml --checkpoint random

--layers SPEC (last | lastN | each | 2,5,-1) takes the features after those encoder blocks, each through the encoder's final LayerNorm,
from one forward pass per batch: the bank and the queries are their concatenation (DINO's last-4 probe: --layers last4), or with
--per_layer one top-k search and vote per block (the per-layer curve: --layers each --per_layer).

    python -m scripts.evaluation.knn_eval --config configs/mae.yaml --checkpoint outputs/pretrain/mae_pretrain/vit-mae.pt --layers each --per_layer
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

import torch
import yaml

from ssrl_vit_mae_jepa_amd.data import STL10_DIR, LabeledBatches, _load_stl10_labeled, get_test_batches, labeled_serving, split_per_class, synthetic_labeled
from ssrl_vit_mae_jepa_amd.representation import KNN_MAX_DIM, config_depth_dim, extract_split_features, knn_topk, knn_vote, load_eval_encoder, parse_ks, parse_layers


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="Weighted k-NN evaluation of a frozen MAE / I-JEPA encoder")
    p.add_argument("--config", type=str, default="configs/mae.yaml")
    p.add_argument("--checkpoint", type=str, required=True, help="checkpoint path (.ckpt / .pt) or 'random'")
    p.add_argument("--encoder", type=str, choices=["target", "context"], default="target", help="I-JEPA encoder (default: the EMA target)")
    p.add_argument("--pool", type=str, choices=["cls", "mean", "cls_mean"], default=None,
                   help="MAE default cls; I-JEPA mean only; cls_mean = [class token | patch mean], with --layers only")
    p.add_argument("--layers", type=str, default=None, help="features after these encoder blocks: last | lastN | each | comma-separated indices")
    p.add_argument("--per_layer", action="store_true", help="with --layers: one k-NN per block instead of one on the concatenation")
    p.add_argument("--normalize", type=str, choices=["l2", "none"], default="l2")
    p.add_argument("--k", type=str, default="10,20,100,200")
    p.add_argument("--temperature", type=float, default=0.07)
    p.add_argument("--samples_per_class", type=int, default=None, help="bank = this many train images per class (split_per_class)")
    p.add_argument("--batch_size", type=int, default=500)
    p.add_argument("--synthetic_images", type=int, default=None, help="use N synthetic labeled images instead of STL-10")
    p.add_argument("--output_dir", type=str, default=None)
    p.add_argument("--save_features", action="store_true", help="also write the bank / query features to <output_dir>/knn_features.pt")
    return p.parse_args(argv)


def bank_split(cfg: dict, samples_per_class, synthetic_images, seed: int = 73):
    """(images uint8, labels, index list, data source) of the bank on the host: the labeled train split, or its per-class
    subset.  Without --synthetic_images the STL-10 files must exist: a synthetic stand-in is never used silently."""
    seed = int(cfg.get("seed", seed))
    if synthetic_images is None:
        loaded = _load_stl10_labeled("train")
        if loaded is None or _load_stl10_labeled("test") is None:
            raise SystemExit(f"knn_eval: the labeled STL-10 files ({STL10_DIR}/train_*.bin, test_*.bin) are missing; "
                             "pass --synthetic_images N to run on synthetic images")
        imgs, labels = loaded
        source = "stl10"
    else:
        imgs, labels = synthetic_labeled(int(synthetic_images), seed=seed)
        source = "synthetic"
    idx = list(range(len(labels))) if samples_per_class is None else split_per_class(labels, int(samples_per_class), seed)[0]
    return imgs, labels, idx, source


def main(argv=None):
    args = parse_args(argv)
    ks = parse_ks(args.k)
    with open(args.config, "r") as f:
        cfg = yaml.safe_load(f)
    model_cfg = cfg["model"]
    is_ijepa = "predictor" in model_cfg
    pool = args.pool or ("mean" if is_ijepa else "cls")
    if is_ijepa and pool != "mean":
        raise SystemExit("knn_eval: I-JEPA encoders see no class token: --pool must be mean")
    layers = None
    if args.layers is not None:
        depth, dim = config_depth_dim(model_cfg)
        try:
            layers = parse_layers(args.layers, depth)
        except ValueError as exc:
            raise SystemExit(f"knn_eval: {exc}")
        width = len(layers) * dim * (2 if pool == "cls_mean" else 1)
        if not args.per_layer and width > KNN_MAX_DIM:  # before any device work
            raise SystemExit(f"knn_eval: {len(layers)} blocks concatenated are {width} columns wide, the k-NN search takes {KNN_MAX_DIM}: "
                             "name fewer blocks or pass --per_layer")
    elif args.per_layer or pool == "cls_mean":
        raise SystemExit("knn_eval: --per_layer and --pool cls_mean need --layers")
    imgs, labels, bank_idx, source = bank_split(cfg, args.samples_per_class, args.synthetic_images)
    if ks[-1] > len(bank_idx):  # before any device work
        raise SystemExit(f"knn_eval: k = {ks[-1]} exceeds the bank size {len(bank_idx)}")
    if not torch.cuda.is_available():
        raise SystemExit("knn_eval: the MI355X engine has no CPU fallback")
    dev = torch.device("cuda", 0)
    bank = LabeledBatches(imgs.to(dev), torch.from_numpy(labels).to(dev), bank_idx, args.batch_size, False, int(cfg.get("seed", 73)),
                          *labeled_serving(cfg))   # the bank at the model's size, as the queries
    precision = cfg.get("engine", {}).get("precision")
    enc = load_eval_encoder(args.checkpoint, model_cfg, encoder=args.encoder, precision=precision, device=dev)
    if not enc.with_cls and pool != "mean":
        raise SystemExit("knn_eval: this checkpoint holds an I-JEPA encoder: --pool must be mean")
    if layers is not None and enc.depth != depth:
        raise SystemExit(f"knn_eval: the encoder has {enc.depth} blocks, the config says {depth}")
    test_cfg = dict(cfg, test=dict(cfg.get("test", {}), batch_size=args.batch_size))
    queries = get_test_batches(test_cfg, dev, synthetic_images=None if args.synthetic_images is None else max(1, args.synthetic_images * 2 // 5))

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    bank_f, bank_y = extract_split_features(enc, bank, pool=pool, normalize=args.normalize, layers=layers)
    query_f, query_y = extract_split_features(enc, queries, pool=pool, normalize=args.normalize, layers=layers)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    num_classes = int(max(int(bank_y.max()), int(query_y.max()))) + 1

    def top1(q, b):
        sims, idx = knn_topk(q, b, ks[-1])
        return {str(k): float((knn_vote(sims, idx, bank_y, num_classes, k=k, temperature=args.temperature, bank_size=b.shape[0]) == query_y).double().mean())
                for k in ks}

    per_layer = None
    if layers is not None and args.per_layer:
        per_layer = {str(l): top1(query_f[:, i].contiguous(), bank_f[:, i].contiguous()) for i, l in enumerate(layers)}
        acc = per_layer[str(layers[-1])]   # top1 = the deepest block named
    else:
        if layers is not None:  # (N, n, W) -> (N, n W): with l2 slices the dot product is the sum of the per-slice cosines
            slices = len(layers) * (2 if pool == "cls_mean" else 1)
            bank_f, query_f = bank_f.flatten(1), query_f.flatten(1)
            if args.normalize == "l2":  # back to unit rows (the mean per-slice cosine), so that --temperature means what it means for one block
                bank_f, query_f = bank_f / slices ** 0.5, query_f / slices ** 0.5
        acc = top1(query_f, bank_f)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    res = dict(checkpoint=args.checkpoint, data=source, kind=enc.kind, encoder=enc.encoder, pool=pool, normalize=args.normalize,
               bank_size=int(bank_f.shape[0]), query_size=int(query_f.shape[0]), temperature=args.temperature, top1=acc,
               extract_images_per_s=(bank_f.shape[0] + query_f.shape[0]) / max(t1 - t0, 1e-9), knn_ms=(t2 - t1) * 1e3)
    if layers is not None:
        res["layers"] = list(layers)
        if per_layer is not None:
            res["per_layer"] = per_layer
    out_dir = Path(args.output_dir) if args.output_dir else Path(cfg.get("logging", {}).get("output_dir_base", "outputs")) / "knn"
    out_dir.mkdir(parents=True, exist_ok=True)
    if args.save_features:
        torch.save({"bank": bank_f.cpu(), "bank_labels": bank_y.cpu(), "queries": query_f.cpu(), "query_labels": query_y.cpu()},
                   out_dir / "knn_features.pt")
    line = json.dumps(res)
    (out_dir / "knn.json").write_text(line + "\n")
    print(line)
    return res


if __name__ == "__main__":
    main()
