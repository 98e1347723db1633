"""What the probe tools (``linear_probe``, ``attentive_probe``) share: the argument checks before any device work, the labeled
batches, the epoch's shuffle, the inner step loop and the evaluation of a split.  Plain functions; each tool keeps its own
epoch-end bookkeeping, because the two write different files.  Losses and counts are length-G device vectors throughout (G heads;
a single probe is G = 1)."""
from __future__ import annotations

import os
import time
from pathlib import Path

import numpy as np
import torch

from ssrl_vit_mae_jepa_amd.data import get_test_batches, get_train_batches

EXTRACT_BATCH = 500   # images per encoder call while extracting


def merge_flags(block, args, flags) -> dict:
    """A YAML block with every given flag of ``flags`` on top."""
    block = dict(block or {})
    for key in flags:
        if getattr(args, key, None) is not None:
            block[key] = getattr(args, key)
    return block


def require_data(tool: str, stl10_dir: Path, synthetic_images) -> None:
    if synthetic_images is not None:
        return
    missing = [n for n in ("train_X.bin", "train_y.bin", "test_X.bin", "test_y.bin") if not (stl10_dir / n).exists()]
    if missing:
        raise SystemExit(f"{tool}: the labeled STL-10 files ({stl10_dir}/train_*.bin, test_*.bin) are missing; "
                         "pass --synthetic_images N to run on synthetic images")


def check_args(tool: str, args, stl10_dir: Path) -> None:
    """The argument errors that end a run before any device work, in the order the tools report them."""
    if args.max_epochs is not None and args.max_epochs < 1:
        raise SystemExit(f"{tool}: --max_epochs must be at least 1")
    if args.checkpoint != "random" and not Path(args.checkpoint).exists():
        raise SystemExit(f"{tool}: checkpoint {args.checkpoint} not found")
    if args.resume is not None and not Path(args.resume).exists():
        raise SystemExit(f"{tool}: --resume {args.resume} not found")
    require_data(tool, stl10_dir, args.synthetic_images)
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: the MI355X engine has no CPU fallback")


def labeled_batches(cfg: dict, args, dev):
    """(data_cfg, train, val, test): the labeled splits served EXTRACT_BATCH images at a time, the training split in its stored order
    (the probe shuffles the cached rows itself); --samples_per_class overrides train.samples_per_class."""
    train_cfg = dict(cfg.get("train") or {}, batch_size=EXTRACT_BATCH)
    if args.samples_per_class is not None:
        train_cfg["samples_per_class"] = int(args.samples_per_class)
    data_cfg = dict(cfg, train=train_cfg, test=dict(cfg.get("test") or {}, batch_size=EXTRACT_BATCH))
    train_b, val_b = get_train_batches(data_cfg, dev, synthetic_images=args.synthetic_images)
    train_b.shuffle = False
    test_b = get_test_batches(data_cfg, dev, synthetic_images=None if args.synthetic_images is None else max(1, args.synthetic_images * 2 // 5))
    return data_cfg, train_b, val_b, test_b


def epoch_batches(n: int, batch: int, seed: int, epoch: int, min_rows: int = 1):
    """Index arrays of the epoch's batches: a permutation of n drawn from (seed, epoch), cut into batches; the last, partial batch is
    used only if it has at least ``min_rows`` rows."""
    order = np.random.default_rng([int(seed), int(epoch)]).permutation(n)
    return [order[i:i + batch] for i in range(0, n, batch) if len(order[i:i + batch]) >= min_rows]


def save(path: Path, obj) -> None:
    tmp = path.with_suffix(path.suffix + ".tmp")
    torch.save(obj, tmp)
    os.replace(tmp, path)


def run_steps(batches, gather, step, dev):
    """The inner loop of an epoch over ``batches`` (``epoch_batches``, at least one): ``gather(i, j)`` gives batch i's (inputs, labels)
    for the device index ``j``, ``step(inputs, labels)`` its (loss (G,), correct (G,)).  Returns (sum of loss x rows (G,) fp64, sum of
    correct (G,) int64, rows, seconds): device vectors, synchronised only around the loop."""
    sync = torch.cuda.synchronize if torch.device(dev).type == "cuda" else (lambda: None)
    loss_sum, correct_sum, rows = 0, 0, 0
    sync()
    t0 = time.perf_counter()
    for i, idx in enumerate(batches):
        loss, correct = step(*gather(i, torch.from_numpy(idx).to(dev)))
        loss_sum = loss_sum + loss.double() * len(idx)
        correct_sum = correct_sum + correct.long()
        rows += len(idx)
    sync()
    return loss_sum, correct_sum, rows, time.perf_counter() - t0


def evaluate_split(probe, inputs: torch.Tensor, labels: torch.Tensor, batch: int):
    """(loss, accuracy) per head over a split, two lists of G floats: the row-weighted mean of ``probe.evaluate``'s batch losses, and
    its correct counts over the rows."""
    n = inputs.shape[0]
    loss, correct = 0, 0
    for i in range(0, n, batch):
        _, l, c = probe.evaluate(inputs[i:i + batch], labels[i:i + batch])
        loss = loss + l.double() * min(batch, n - i)
        correct = correct + c.long()
    return [v / n for v in loss.tolist()], [v / n for v in correct.tolist()]
