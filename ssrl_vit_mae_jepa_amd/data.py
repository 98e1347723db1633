"""Input step before the hot path: batches of (B, 3, S, S) images at the model's size S, uint8 as the dataset stores them, on the GPU.

Mirrors what the reference's ``get_pretrain_dataloaders`` (src/data.py:45-106) hands the step, without torchvision
(not installed): the STL-10 unlabeled split is read straight from its binary file (uint8, column-major images) and kept
uint8 all the way INTO the engine (27.6 KB/image instead of 110.6 KB fp32): ToTensor + Normalize(.5,.5)
(src/data.py:22-23) is applied by the kernels that read pixels (csrc/k_pixels.hip), bit-identical to the torch
expression ``normalize_u8``.  The dataset lives either on the device (``engine.data_on_device: true``, the default:
2.6 GB for STL-10 unlabeled) or in pinned host memory, streamed by ``PinnedBatchStream``: index gather on the host into
a pinned staging buffer, H2D copy on a side stream into one of two device buffers, so batch i+1 crosses PCIe while
batch i trains (55 MB per 2000-image batch: 0.9 ms at 63 GB/s against a 25 ms step).
The 94 000 / 6 000 split uses ``random_split``'s permutation with generator seed 73 (src/data.py:74-80).
Augmentation follows what the reference actually does, quirk included (src/data.py:74-81): ``val_subset.dataset`` is the
object ``random_split`` was given, so with data_fraction == 1.0 the assignment overwrites the shared STL10 transform and
BOTH loaders serve un-augmented images, while with data_fraction < 1.0 it lands on the ``Subset`` wrapper, does nothing,
and BOTH loaders keep the training transform RandomResizedCrop(96, scale=(0.8, 1.0)) + RandomHorizontalFlip
(src/data.py:18-21).  That transform is applied here on the GPU to whole batches (crop box sampled like torchvision's
``get_params``, bilinear resampling through an affine grid, flip by sign of the x scale); it cannot be bit-identical to
PIL's fixed-point resize nor share its RNG stream, so it is the same distribution, not the same pixels.
Without the dataset file (no network here) it serves seeded synthetic uniform[-1,1] images of the same shape.
A model of another size than the dataset (``model.general.image_size`` != 96: ViT-B/16 and ViT-L/14 at 224 px) is fed through
``resize_batch`` (csrc/k_resize.hip, ``mae_resize_crop_flip``): the dataset stays resident at 96 px uint8 -- on the device or in
pinned memory -- and every batch takes ONE pass that crops, flips and resamples it to the model's size, the reference's
RandomResizedCrop(size) for training and Resize(size) + CenterCrop(size) for evaluation (src/data.py:15-34; a square image has
nothing to centre-crop).  The crop box is drawn at the source size by the unchanged ``draw_augment_params``, so data-parallel
ranks still agree; the batch leaves as uint8 where the engine reads bytes and as normalised fp32 otherwise (``serves_u8``).
The labeled loaders do the same with the plain whole-image resize (``LabeledBatches(image_size=...)``); a configuration of
the dataset's own size, or one without a model block, takes none of this: the old kernel, the old path, the old bits.
"""
from __future__ import annotations

from pathlib import Path
import math
from typing import Callable, Iterator, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

STL10_UNLABELED = Path("data") / "stl10_binary" / "unlabeled_X.bin"


def _load_stl10_unlabeled(path: Path, fraction: float) -> torch.Tensor:
    raw = np.memmap(path, dtype=np.uint8, mode="r")
    n = raw.size // (3 * 96 * 96)
    n_use = int(n * fraction) if fraction < 1.0 else n
    imgs = np.asarray(raw[: n_use * 3 * 96 * 96]).reshape(n_use, 3, 96, 96)
    return torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 1, 3, 2)))  # file stores each plane column-major


def normalize_u8(x: torch.Tensor) -> torch.Tensor:
    """ToTensor (x/255) then Normalize(mean .5, std .5): (x/255 - .5)/.5, fp32."""
    return (x.to(torch.float32) / 255.0 - 0.5) / 0.5


def random_resized_crop_params(n: int, size: int, gen: torch.Generator, scale=(0.8, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """torchvision RandomResizedCrop.get_params for n square images at once: up to 10 draws of (area, log-uniform aspect),
    the first whose box fits is kept, otherwise the whole image (ratio is inside the bounds for a square).  Returns
    integer (top, left, h, w) tensors on the generator's device."""
    dev = gen.device
    area = float(size * size)
    top = torch.zeros(n, dtype=torch.int64, device=dev); left = torch.zeros_like(top)
    h = torch.full_like(top, size); w = torch.full_like(top, size)
    done = torch.zeros(n, dtype=torch.bool, device=dev)
    log_lo, log_hi = float(np.log(ratio[0])), float(np.log(ratio[1]))
    for _ in range(10):
        target = area * (scale[0] + (scale[1] - scale[0]) * torch.rand(n, generator=gen, device=dev))
        ar = torch.exp(log_lo + (log_hi - log_lo) * torch.rand(n, generator=gen, device=dev))
        cw = torch.round(torch.sqrt(target * ar)).to(torch.int64)
        ch = torch.round(torch.sqrt(target / ar)).to(torch.int64)
        ok = (cw > 0) & (cw <= size) & (ch > 0) & (ch <= size) & ~done
        u, v = torch.rand(n, generator=gen, device=dev), torch.rand(n, generator=gen, device=dev)
        t = torch.floor(u * (size - ch + 1).clamp_min(1)).to(torch.int64)   # randint(0, size - h + 1)
        l = torch.floor(v * (size - cw + 1).clamp_min(1)).to(torch.int64)
        top = torch.where(ok, t, top); left = torch.where(ok, l, left)
        h = torch.where(ok, ch, h); w = torch.where(ok, cw, w)
        done |= ok
    return top, left, h, w


def augment_batch(x: torch.Tensor, gen: Optional[torch.Generator] = None, params=None) -> torch.Tensor:
    """RandomResizedCrop(size, scale=(0.8, 1.0)) + RandomHorizontalFlip() on a (B, C, S, S) float batch, on its device
    (``params``: the output of ``draw_augment_params`` sliced to the batch's rows, instead of drawing them here)."""
    import torch.nn.functional as F
    B, _, S, _ = x.shape
    if params is None:
        top, left, h, w = random_resized_crop_params(B, S, gen)
        flip = torch.rand(B, generator=gen, device=gen.device) < 0.5
    else:
        top, left, h, w, flip = params
    # affine grid in normalised coordinates (align_corners=False): output pixel centres map to the crop box
    sx = w.to(torch.float32) / S; sy = h.to(torch.float32) / S
    cx = (2.0 * left.to(torch.float32) + w.to(torch.float32)) / S - 1.0
    cy = (2.0 * top.to(torch.float32) + h.to(torch.float32)) / S - 1.0
    sx = torch.where(flip, -sx, sx)
    theta = torch.zeros(B, 2, 3, device=x.device)
    theta[:, 0, 0] = sx.to(x.device); theta[:, 0, 2] = cx.to(x.device)
    theta[:, 1, 1] = sy.to(x.device); theta[:, 1, 2] = cy.to(x.device)
    grid = F.affine_grid(theta, list(x.shape), align_corners=False)
    return F.grid_sample(x, grid, mode="bilinear", padding_mode="border", align_corners=False)


def draw_augment_params(n: int, size: int, gen: torch.Generator):
    """Crop boxes and flips of n images: (top, left, h, w, flip) integer tensors on the generator's device.  Drawn for the
    GLOBAL batch on every rank (five numbers per image) and sliced to the rank's rows, so that a data-parallel run augments
    every image exactly as the one-GPU run does."""
    top, left, h, w = random_resized_crop_params(n, size, gen)
    flip = torch.rand(n, generator=gen, device=gen.device) < 0.5
    return top, left, h, w, flip


def augment_batch_u8(x: torch.Tensor, gen: Optional[torch.Generator] = None, params=None) -> torch.Tensor:
    """The same augmentation on a uint8 device batch, by the HIP kernel behind ``mae_augment_crop_flip_u8`` (uint8 in, uint8
    out, as the reference's PIL transforms run before ToTensor): the crop boxes and flips are drawn here with the rule of
    ``random_resized_crop_params`` (or passed in as ``params``, already sliced to the batch's rows), the resampling runs in
    libmae_hip.so.  No torch fallback: a missing extension fails loudly."""
    from ._lib import check, lib, ptr
    from .mae import _stream
    if x.dtype != torch.uint8 or not x.is_cuda or x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"augment_batch_u8 needs a square (B, C, S, S) uint8 CUDA batch, got {tuple(x.shape)} {x.dtype} on {x.device}")
    B, C, S, _ = x.shape
    top, left, h, w, flip = draw_augment_params(B, S, gen) if params is None else params
    params = torch.stack([top, left, h, w, flip.to(torch.int64)], dim=1).to(device=x.device, dtype=torch.int32).contiguous()
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib.mae_augment_crop_flip_u8(ptr(x), ptr(params), B, C, S, ptr(out), _stream(x.device)))
    return out


DATASET_SIZE = 96   # STL-10 and its synthetic stand-ins: the resolution every loader keeps the dataset at


def model_image_size(cfg: dict) -> int:
    """``model.general.image_size`` of a configuration; one without a model block serves the dataset's own resolution."""
    return int((cfg.get("model") or {}).get("general", {}).get("image_size", DATASET_SIZE))


def serves_u8(cfg: dict) -> bool:
    """Whether the model of a configuration reads raw bytes: the uint8 pixel kernels take patch sizes that are multiples of 4
    on grids up to 64 x 64 (csrc/k_pixels.hip); other geometries (the reference class's default patch_size 6, ViT-L/14) are
    served normalised fp32 batches, which every engine kernel accepts."""
    general = (cfg.get("model") or {}).get("general", {})
    patch = int(general.get("patch_size", 8))
    return patch % 4 == 0 and model_image_size(cfg) // max(1, patch) <= 64


def check_boxes(params: torch.Tensor, size: int) -> None:
    """ValueError unless every row (top, left, h, w, flip) of a host tensor is a box inside a size x size image."""
    if params.dim() != 2 or params.shape[1] != 5:
        raise ValueError(f"crop parameters must be (B, 5) rows of (top, left, h, w, flip), got {tuple(params.shape)}")
    p = params.to(torch.int64)
    top, left, h, w = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    bad = (top < 0) | (left < 0) | (h < 1) | (w < 1) | (top + h > size) | (left + w > size)
    if bool(bad.any()):
        b = int(bad.nonzero()[0])
        raise ValueError(f"crop box {p[b, :4].tolist()} of image {b} does not lie inside a {size} x {size} image")


def resize_batch(x: torch.Tensor, out_size: int, params=None, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """A square (B, C, S, S) uint8 or float32 device batch resampled to (B, C, out_size, out_size) by the HIP kernel behind
    ``mae_resize_crop_flip``: bilinear where an axis keeps or gains pixels, the antialiasing triangle filter where it loses
    them (``F.interpolate(mode="bilinear", antialias=True)`` for the whole image).  ``params``: None (the whole image), the
    (top, left, h, w, flip) tuple of ``draw_augment_params`` sliced to the batch's rows, or a (B, 5) integer tensor -- boxes in
    source pixels, resampled straight to ``out_size`` with the columns mirrored under a flip.  Host boxes are validated here
    (a box outside the image is a ValueError); device boxes are clamped by the kernel, never read out of bounds.
    ``out_dtype``: uint8 input gives uint8 (default) or normalised float32, bit-identical to ``normalize_u8`` of the uint8
    result; float32 input gives float32, not normalised.  No torch fallback: a missing extension fails loudly."""
    from . import _lib
    from ._lib import check, lib, ptr
    from .mae import _stream
    if x.dtype not in (torch.uint8, torch.float32) or not x.is_cuda or x.dim() != 4 or x.shape[2] != x.shape[3]:
        raise ValueError(f"resize_batch needs a square (B, C, S, S) uint8 or float32 CUDA batch, got {tuple(x.shape)} {x.dtype} on {x.device}")
    B, C, S, _ = x.shape
    out_size = int(out_size)
    if out_dtype is None:
        out_dtype = x.dtype
    if out_dtype not in (torch.uint8, torch.float32) or (out_dtype == torch.uint8 and x.dtype != torch.uint8):
        raise ValueError(f"resize_batch: {x.dtype} input cannot leave as {out_dtype}")
    if out_size < 1 or S > 8 * out_size:
        raise ValueError(f"resize_batch: out_size {out_size} must be positive and at least an eighth of the input size {S}")
    if params is not None:
        if not torch.is_tensor(params):
            top, left, h, w, flip = params
            params = torch.stack([top, left, h, w, flip.to(top.dtype)], dim=1)
        if params.shape[0] != B:
            raise ValueError(f"resize_batch: {params.shape[0]} crop boxes for a batch of {B}")
        if not params.is_cuda:
            check_boxes(params, S)
        params = params.to(device=x.device, dtype=torch.int32).contiguous()
    x = x.contiguous()
    out = torch.empty((B, C, out_size, out_size), dtype=out_dtype, device=x.device)
    if B == 0:
        return out
    dt = lambda d: _lib.MAE_U8 if d == torch.uint8 else _lib.MAE_F32  # noqa: E731
    check(lib.mae_resize_crop_flip(ptr(x), dt(x.dtype), B, C, S, ptr(params), out_size, dt(out_dtype), ptr(out), _stream(x.device)))
    return out


def augment_to_size(x: torch.Tensor, out_size: Optional[int], params, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """RandomResizedCrop(out_size) + flip of a uint8 device batch with boxes drawn at ITS size: ``augment_batch_u8`` (the same
    bits as ever) when the size stays (``out_size`` None or the batch's own), one ``resize_batch`` pass when it changes."""
    if out_size is None or (out_size == x.shape[-1] and out_dtype in (None, torch.uint8)):
        return augment_batch_u8(x, params=params)
    return resize_batch(x, out_size, params=params, out_dtype=out_dtype)


class PinnedBatchStream:
    """uint8 dataset in pinned host memory -> device batches through two device buffers (double buffering).

    ``batches(order)`` yields ``data[order[i:i+batch]]`` as device tensors.  While the consumer works on buffer s, the next
    batch is gathered on the host into pinned staging buffer 1-s and copied on ``copy_stream``; the consumer's stream waits
    for the copy's event (never the host), and a buffer is rewritten only after the kernels that read it have finished
    (an event recorded on the consumer's stream when the next batch is requested)."""

    def __init__(self, data_u8: torch.Tensor, batch: int, device: torch.device):
        if data_u8.dtype != torch.uint8 or data_u8.is_cuda:
            raise ValueError("PinnedBatchStream takes a uint8 host tensor")
        self.device, self.batch = device, int(batch)
        self.data = data_u8.contiguous()
        shape = (self.batch,) + tuple(data_u8.shape[1:])
        self.stage = [torch.empty(shape, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self.dev = [torch.empty(shape, dtype=torch.uint8, device=device) for _ in range(2)]
        self.copy_stream = torch.cuda.Stream(device=device)
        self.ready = [torch.cuda.Event() for _ in range(2)]
        self.free = [torch.cuda.Event() for _ in range(2)]
        self.staged = [torch.cuda.Event() for _ in range(2)]   # the H2D copy out of a staging buffer has finished
        self._used = [False, False]

    def _submit(self, slot: int, idx: torch.Tensor) -> int:
        n = idx.numel()
        if self._used[slot]:
            self.staged[slot].synchronize()  # host: the previous copy out of this staging buffer is done
        torch.index_select(self.data, 0, idx, out=self.stage[slot][:n])
        with torch.cuda.stream(self.copy_stream):
            if self._used[slot]:
                self.copy_stream.wait_event(self.free[slot])  # device: the consumer finished with this buffer
            self.dev[slot][:n].copy_(self.stage[slot][:n], non_blocking=True)
            self.staged[slot].record(self.copy_stream)
            self.ready[slot].record(self.copy_stream)
        self._used[slot] = True
        return n

    def batches(self, order: torch.Tensor) -> Iterator[torch.Tensor]:
        order = order.to("cpu", torch.int64)
        return self.batches_of([order[i:i + self.batch] for i in range(0, order.numel(), self.batch)])

    def batches_of(self, chunks) -> Iterator[torch.Tensor]:
        """The same pipeline over explicit index chunks (each at most ``batch`` long; a chunk may be empty: a data-parallel rank's
        share of a short last batch)."""
        chunks = [c.to("cpu", torch.int64) for c in chunks]
        if not chunks:
            return
        n_next = self._submit(0, chunks[0])
        for i in range(len(chunks)):
            slot, n = i & 1, n_next
            if i + 1 < len(chunks):
                n_next = self._submit(1 - slot, chunks[i + 1])  # overlaps whatever the consumer enqueued for batch i-1
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self.ready[slot])
            yield self.dev[slot][:n]
            self.free[slot].record(torch.cuda.current_stream(self.device))  # everything the consumer enqueued on it so far


class ShardedBatch:
    """What the training loops get per step under data parallelism: THIS rank's rows of a global batch (fetched / copied /
    augmented for these rows only), the global row count and the rank's row range inside it."""
    __slots__ = ("images", "global_rows", "lo", "hi")

    def __init__(self, images: torch.Tensor, global_rows: int, lo: int, hi: int):
        self.images, self.global_rows, self.lo, self.hi = images, int(global_rows), int(lo), int(hi)


def accumulation_plan(n_rows: int, batch: int, accumulate: int) -> List[List[int]]:
    """The row counts of one epoch's micro-batches, grouped into the windows that feed one optimizer step each
    (``accumulate_grad_batches``): ``n_rows`` rows in micro-batches of ``batch``, ``accumulate`` consecutive ones per window.
    No batch is dropped (src/data.py:86-92) and no window spans epochs, so the last window may hold fewer micro-batches and a
    short last one.  The loops read a window's row total from here instead of holding its batches back."""
    n_rows, batch, accumulate = int(n_rows), int(batch), int(accumulate)
    if n_rows < 0 or batch < 1 or accumulate < 1:
        raise ValueError(f"accumulation_plan needs n_rows >= 0, batch >= 1 and accumulate >= 1, got {(n_rows, batch, accumulate)}")
    micro = [min(batch, n_rows - i) for i in range(0, n_rows, batch)]
    return [micro[i:i + accumulate] for i in range(0, len(micro), accumulate)]


def accumulation_slots(plan: List[List[int]]) -> List[Tuple[int, int, int, int]]:
    """``accumulation_plan`` per micro-batch, in the order a loader serves them: (index in its window, micro-batches of the
    window, rows of the window, rows of the window before this micro-batch)."""
    return [(i, len(w), sum(w), sum(w[:i])) for w in plan for i in range(len(w))]


def get_pretrain_batches(cfg: dict, device: torch.device, synthetic_images: Optional[int] = None, seed: int = 73, rank: int = 0,
                         world: int = 1) -> Tuple[Callable[[int], Iterator["ShardedBatch"]], Callable[[], Iterator["ShardedBatch"]]]:
    """(train_batches(epoch), val_batches()): iterators of ``ShardedBatch``.  The order of the global batches and their
    augmentation parameters do not depend on the world size; rank r fetches rows [gb r / W, gb (r + 1) / W) of each global
    batch only (the last batch of an epoch may be ragged: no batch is dropped, as in the reference, src/data.py:86-92).
    ``train_batches.steps_per_epoch`` = global batches per epoch."""
    pre = cfg["pretrain"]
    batch = int(pre.get("batch_size", 512))
    val_split = float(pre.get("val_split", 0.1))
    fraction = float(pre.get("data_fraction", 1.0))
    seed = int(cfg.get("seed", seed))
    on_device = bool(cfg.get("engine", {}).get("data_on_device", True))
    patch = int(cfg.get("model", {}).get("general", {}).get("patch_size", 8))
    img_size = int(cfg.get("model", {}).get("general", {}).get("image_size", 96))
    # the uint8 pixel kernels take patch sizes that are multiples of 4 (csrc/k_pixels.hip); other geometries (the reference
    # class's default patch_size 6, ViT-L/14) are served normalised fp32 batches, which every engine kernel accepts
    keep_u8 = patch % 4 == 0 and img_size // max(1, patch) <= 64
    stream: Optional[PinnedBatchStream] = None
    if synthetic_images is None and STL10_UNLABELED.exists():
        host = _load_stl10_unlabeled(STL10_UNLABELED, fraction)
        n_total = host.shape[0]
        if on_device:
            data = host.to(device)  # uint8 on device; the engine normalises while it reads
            fetch = lambda idx: data[idx]  # noqa: E731
        else:
            stream = PinnedBatchStream(host.pin_memory(), (batch + world - 1) // world + 1, device)
            fetch = None
    else:
        n_total = int(synthetic_images or 4 * batch)
        g = torch.Generator(device=device).manual_seed(seed)
        data = (torch.rand(n_total, 3, 96, 96, device=device, generator=g) * 2 - 1)
        fetch = lambda idx: data[idx]  # noqa: E731
    n_val = int(n_total * val_split)
    n_train = n_total - n_val
    perm = torch.randperm(n_total, generator=torch.Generator().manual_seed(seed))  # random_split's permutation
    idx_dev = torch.device("cpu") if stream is not None else device
    train_idx, val_idx = perm[:n_train].to(idx_dev), perm[n_train:].to(idx_dev)
    if rank == 0:
        print(f"Unlabeled pretrain split: {n_train} train, {n_val} val ({val_split * 100:.1f}% validation)")

    augment = fraction < 1.0  # the reference's quirk: see the module docstring
    aug_gen = torch.Generator(device=device).manual_seed(seed + 7)

    def finish(x: torch.Tensor, lo: int, hi: int, gb: int) -> torch.Tensor:
        params = None
        if img_size != x.shape[-1]:
            # a model of another size than the dataset: the box is drawn at the SOURCE size by the same rule and generator (so the
            # ranks still agree) and resampled straight to the model's size, in the one pass that also resizes
            if augment:
                params = tuple(t[lo:hi] for t in draw_augment_params(gb, x.shape[-1], aug_gen))
            out_dt = torch.uint8 if (x.dtype == torch.uint8 and keep_u8) else torch.float32
            return resize_batch(x, img_size, params=params, out_dtype=out_dt)
        if hi == lo:   # this rank holds no row of a short last batch (the generator still advances below, in step with the other ranks)
            if augment:
                draw_augment_params(gb, x.shape[-1], aug_gen)
            return (x if (x.dtype == torch.uint8 and keep_u8) else normalize_u8(x) if x.dtype == torch.uint8 else x).contiguous()
        if augment:  # parameters of the whole global batch (cheap), this rank's rows of them
            params = tuple(t[lo:hi] for t in draw_augment_params(gb, x.shape[-1], aug_gen))
        if x.dtype == torch.uint8 and x.is_cuda and keep_u8:
            return augment_batch_u8(x, params=params) if augment else x.contiguous()  # uint8 stays uint8: normalised inside the engine
        x = normalize_u8(x) if x.dtype == torch.uint8 else x
        return (augment_batch(x, params=params) if augment else x).contiguous()

    def shards(order: torch.Tensor):
        from .dist import shard_bounds
        for i in range(0, order.numel(), batch):  # no drop_last, like the reference
            idx = order[i:i + batch]
            lo, hi = shard_bounds(idx.numel(), rank, world)
            yield idx[lo:hi], idx.numel(), lo, hi

    def serve(order: torch.Tensor) -> Iterator[ShardedBatch]:
        if stream is not None:
            plan = list(shards(order))
            for (idx, gb, lo, hi), x in zip(plan, stream.batches_of([p[0] for p in plan])):
                yield ShardedBatch(finish(x, lo, hi, gb), gb, lo, hi)
        else:
            for idx, gb, lo, hi in shards(order):
                yield ShardedBatch(finish(fetch(idx), lo, hi, gb), gb, lo, hi)

    def train_batches(epoch: int) -> Iterator[ShardedBatch]:
        g = torch.Generator().manual_seed(seed + 1000 + epoch)  # DataLoader(shuffle=True): a fresh order per epoch
        return serve(train_idx[torch.randperm(n_train, generator=g).to(train_idx.device)])

    def val_batches() -> Iterator[ShardedBatch]:
        return serve(val_idx)

    train_batches.steps_per_epoch = (n_train + batch - 1) // batch
    train_batches.n_train = n_train
    return train_batches, val_batches


# ---------------------------------------------------------------------------------------------------------------------
# Labeled STL-10 (fine-tuning / evaluation: src/data.py:109-176)
# ---------------------------------------------------------------------------------------------------------------------
STL10_DIR = Path("data") / "stl10_binary"


def _load_stl10_labeled(split: str) -> Optional[Tuple[torch.Tensor, np.ndarray]]:
    xp, yp = STL10_DIR / f"{split}_X.bin", STL10_DIR / f"{split}_y.bin"
    if not (xp.exists() and yp.exists()):
        return None
    raw = np.fromfile(xp, dtype=np.uint8)
    imgs = raw.reshape(-1, 3, 96, 96).transpose(0, 1, 3, 2)  # file stores each plane column-major
    labels = np.fromfile(yp, dtype=np.uint8).astype(np.int64) - 1  # STL-10 labels 1..10 -> 0..9 (torchvision STL10)
    return torch.from_numpy(np.ascontiguousarray(imgs)), labels


def split_per_class(labels: np.ndarray, samples_per_class: int, seed: int = 73) -> Tuple[List[int], List[int]]:
    """src/data.py:129-138: for each class in sorted order, its indices shuffled by a FRESH default_rng(seed); the first
    samples_per_class go to train, the rest to validation (lists in that class-major order)."""
    train_idx: List[int] = []
    val_idx: List[int] = []
    for c in np.unique(labels):
        cls_idx = np.where(labels == c)[0]
        np.random.default_rng(seed).shuffle(cls_idx)
        train_idx.extend(cls_idx[:samples_per_class].tolist())
        val_idx.extend(cls_idx[samples_per_class:].tolist())
    return train_idx, val_idx


def synthetic_labeled(n: int, num_classes: int = 10, seed: int = 73) -> Tuple[torch.Tensor, np.ndarray]:
    """Seeded stand-in for a labeled split: balanced labels (i mod num_classes, shuffled) and uint8 images whose class is
    recoverable from the pixels -- a class-dependent low-frequency grating (orientation and phase fixed per class, the
    same in every split) plus seeded noise."""
    g = torch.Generator().manual_seed(seed)
    labels = (torch.arange(n) % num_classes)[torch.randperm(n, generator=g)]
    yy, xx = torch.meshgrid(torch.arange(96, dtype=torch.float32), torch.arange(96, dtype=torch.float32), indexing="ij")
    ang = torch.arange(num_classes, dtype=torch.float32) * (math.pi / num_classes)
    freq = 2 * math.pi * 3 / 96
    pat = torch.sin(freq * (xx[None] * torch.cos(ang)[:, None, None] + yy[None] * torch.sin(ang)[:, None, None]))  # (K, 96, 96)
    chan = torch.tensor([1.0, -0.5, 0.25])[None, :, None, None]
    base = 128 + 70 * pat[labels][:, None] * chan
    imgs = (base + 25 * torch.randn(n, 3, 96, 96, generator=g)).clamp(0, 255).round().to(torch.uint8)
    return imgs, labels.numpy().astype(np.int64)


class LabeledBatches:
    """(images uint8 on the device, labels int64 on the device) batches of a fixed index list; ``shuffle`` reorders the
    list every epoch from a generator seeded with (seed, epoch) (DataLoader(shuffle=True)); no batch is dropped.
    ``image_size`` other than the stored resolution: the split stays resident as stored and every batch leaves through the plain
    whole-image ``resize_batch`` (Resize(size) + CenterCrop(size) of a square image, src/data.py:25-34), as ``out_dtype``
    (None: uint8)."""

    def __init__(self, images: torch.Tensor, labels: torch.Tensor, idx: List[int], batch: int, shuffle: bool, seed: int,
                 image_size: Optional[int] = None, out_dtype: Optional[torch.dtype] = None):
        self.images, self.labels = images, labels
        self.image_size, self.out_dtype = (None if image_size is None else int(image_size)), out_dtype
        self.idx = torch.as_tensor(idx, dtype=torch.int64, device=images.device)
        self.batch, self.shuffle, self.seed = int(batch), shuffle, seed
        self.n = len(idx)
        self.steps_per_epoch = (self.n + self.batch - 1) // self.batch

    def __call__(self, epoch: int = 0) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        order = self.idx
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + 1000 + epoch)
            order = order[torch.randperm(self.n, generator=g).to(order.device)]
        for i in range(0, self.n, self.batch):
            j = order[i:i + self.batch]
            x = self.images[j].contiguous()
            if self.image_size is not None and self.image_size != x.shape[-1]:
                x = resize_batch(x, self.image_size, out_dtype=self.out_dtype)
            yield x, self.labels[j].contiguous()


def labeled_serving(cfg: dict):
    """(image_size, out_dtype) the labeled loaders serve for a configuration: the model's size, uint8 where its engine reads
    bytes; (None, None) -- batches as stored -- for the dataset's own size or a configuration without a model block."""
    size = model_image_size(cfg)
    if size == DATASET_SIZE:
        return None, None
    return size, (torch.uint8 if serves_u8(cfg) else torch.float32)


def get_train_batches(cfg: dict, device: torch.device, synthetic_images: Optional[int] = None, seed: int = 73,
                      train_at_dataset_size: bool = False):
    """(train_batches(epoch), val_batches()) over the labeled STL-10 train split (``train_X.bin`` / ``train_y.bin``),
    split per class as src/data.py:126-138 does.  Neither split is augmented: the reference assigns the eval transform to
    ``val_dataset.dataset`` (src/data.py:139), which is the STL10 object BOTH subsets share, so its training images are only
    normalised too; the same holds here (uint8 on the device, normalised inside the engine's pixel kernels).  Without the
    files: ``synthetic_labeled`` images (default 5000), with samples_per_class capped at 80 % of a class.
    Both loaders serve batches of ``model.general.image_size`` (resized on the device, see ``LabeledBatches``).
    ``train_at_dataset_size``: the TRAINING loader alone keeps the dataset's resolution, for a consumer that resizes itself after
    its own per-image augmentation (``train.augment``: the ops run on the stored bytes, the resize follows)."""
    train_cfg = cfg["train"]
    seed = int(cfg.get("seed", seed))
    spc = int(train_cfg.get("samples_per_class", 400))
    loaded = None if synthetic_images is not None else _load_stl10_labeled("train")
    if loaded is None:
        n = int(synthetic_images or 5000)
        imgs, labels = synthetic_labeled(n, seed=seed)
        spc = min(spc, int(0.8 * n / 10))
    else:
        imgs, labels = loaded
    train_idx, val_idx = split_per_class(labels, spc, seed)
    print(f"Using {spc} samples/class -> {len(train_idx)} train, {len(val_idx)} val")
    images = imgs.to(device)
    lab = torch.from_numpy(labels).to(device)
    bs = int(train_cfg.get("batch_size", 64))
    size, out_dt = labeled_serving(cfg)
    return (LabeledBatches(images, lab, train_idx, bs, True, seed, None if train_at_dataset_size else size, out_dt),
            LabeledBatches(images, lab, val_idx, bs, False, seed, size, out_dt))


def get_test_batches(cfg: dict, device: torch.device, synthetic_images: Optional[int] = None, seed: int = 73) -> LabeledBatches:
    """The labeled STL-10 test split (``test_X.bin`` / ``test_y.bin``) in file order (src/data.py:157-176); without the
    files, ``synthetic_labeled`` images drawn with another seed than the training split's.  Batches of
    ``model.general.image_size``, as ``get_train_batches`` serves them."""
    loaded = None if synthetic_images is not None else _load_stl10_labeled("test")
    if loaded is None:
        imgs, labels = synthetic_labeled(int(synthetic_images or 2000), seed=int(cfg.get("seed", seed)) + 1)
    else:
        imgs, labels = loaded
    bs = int(cfg.get("test", {}).get("batch_size", 64))
    return LabeledBatches(imgs.to(device), torch.from_numpy(labels).to(device), list(range(len(labels))), bs, False, seed, *labeled_serving(cfg))


# ---------------------------------------------------------------------------------------------------------------------
# mixup / CutMix for fine-tuning (timm.data.Mixup, mode="batch"; MAE main_finetune.py: mixup 0.8, cutmix 1.0, prob 1, switch 0.5)
# ---------------------------------------------------------------------------------------------------------------------
class MixParams(NamedTuple):
    """One batch's draw, host tensors: ``partner`` (B) int32, ``lam`` (B) fp32, ``box`` (B, 4) int32 (y0, y1, x0, x1),
    ``cutmix`` True when the batch is pure CutMix (nothing is blended outside the box)."""
    partner: torch.Tensor
    lam: torch.Tensor
    box: torch.Tensor
    cutmix: bool

    @property
    def identity(self) -> bool:
        """lam = 1 and an empty box in a host draw: the mixed batch is the batch (a device draw is never inspected: no sync)."""
        if self.cutmix or self.lam.is_cuda or self.box.is_cuda:
            return False
        return bool((self.lam == 1).all()) and bool((self.box[:, 0] >= self.box[:, 1]).logical_or(self.box[:, 2] >= self.box[:, 3]).all())


def draw_mix_params(batch: int, size: int, gen_or_seed: Union[np.random.Generator, int, Sequence[int]], mixup_alpha: float = 0.8,
                    cutmix_alpha: float = 1.0, prob: float = 1.0, switch_prob: float = 0.5) -> MixParams:
    """timm's ``Mixup._params_per_batch`` + ``cutmix_bbox_and_lam`` (correct_lam=True) for one batch of square images:
    with probability ``prob`` the batch is mixed -- CutMix with probability ``switch_prob`` when both alphas are positive
    (the one positive alpha decides otherwise) -- with ONE lam ~ Beta(alpha, alpha) for the whole batch.  CutMix cuts the box
    of ratio sqrt(1 - lam): cut = int(S * ratio), centre randint(0, S) per axis, edges clip(c -+ cut // 2, 0, S), and lam
    becomes 1 - area / S^2.  The partner of image b is b flipped, B - 1 - b.  ``gen_or_seed``: a numpy Generator, or the
    entropy of one (an int, or a tuple such as (seed, epoch, step): the same numbers give the same draw).  Host arithmetic
    only: nothing here touches the device."""
    rng = gen_or_seed if isinstance(gen_or_seed, np.random.Generator) else np.random.default_rng(gen_or_seed)
    B, S = int(batch), int(size)
    lam, cutmix = 1.0, False
    box = (0, 0, 0, 0)
    if (mixup_alpha > 0 or cutmix_alpha > 0) and rng.random() < prob:
        if mixup_alpha > 0 and cutmix_alpha > 0:
            cutmix = bool(rng.random() < switch_prob)
        else:
            cutmix = cutmix_alpha > 0
        alpha = cutmix_alpha if cutmix else mixup_alpha
        lam = float(rng.beta(alpha, alpha))
        if cutmix:
            cut = int(S * math.sqrt(1.0 - lam))
            cy, cx = int(rng.integers(0, S)), int(rng.integers(0, S))
            y0, y1 = int(np.clip(cy - cut // 2, 0, S)), int(np.clip(cy + cut // 2, 0, S))
            x0, x1 = int(np.clip(cx - cut // 2, 0, S)), int(np.clip(cx + cut // 2, 0, S))
            box = (y0, y1, x0, x1)
            lam = 1.0 - ((y1 - y0) * (x1 - x0)) / float(S * S)
    return MixParams(partner=torch.arange(B - 1, -1, -1, dtype=torch.int32),
                     lam=torch.full((B,), lam, dtype=torch.float64).to(torch.float32),
                     box=torch.tensor(box, dtype=torch.int32).repeat(B, 1), cutmix=cutmix)


def mix_batch(images: torch.Tensor, labels: torch.Tensor, params: MixParams):
    """The batch mixed by the HIP kernel behind ``mae_mix_batch``: returns (mixed, ya, yb, lam) on the images' device with
    ya = labels, yb = labels[partner], lam the (B) fp32 weights of ya.  Pure CutMix on a uint8 batch stays uint8 (the engine
    keeps reading 1 byte per pixel); everything else leaves as normalised fp32.  An identity draw returns the batch itself.
    A host draw (what ``draw_mix_params`` returns) reaches the device through pinned memory: no host-device synchronisation;
    one whose tensors are already on the device is used as it is.  No torch fallback."""
    from . import _lib
    from ._lib import check, lib, ptr
    from .mae import _stream
    if images.dtype not in (torch.uint8, torch.float32) or not images.is_cuda or images.dim() != 4 or images.shape[2] != images.shape[3]:
        raise ValueError(f"mix_batch needs a square (B, C, S, S) uint8 or float32 CUDA batch, got {tuple(images.shape)} {images.dtype} on {images.device}")
    B, C, S, _ = images.shape
    if params.partner.shape != (B,) or params.lam.shape != (B,) or params.box.shape != (B, 4) or labels.shape != (B,):
        raise ValueError(f"mix_batch: labels / parameters are not those of a batch of {B}")
    dev = images.device
    def up(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:  # a draw already on the device passes through
        t = t.to(dt).contiguous()
        return t.to(dev) if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)
    lam = up(params.lam, torch.float32)
    if params.identity:
        return images, labels, labels, lam
    partner, box = up(params.partner, torch.int32), up(params.box, torch.int32)
    images = images.contiguous()
    u8_out = params.cutmix and images.dtype == torch.uint8
    out = torch.empty((B, C, S, S), dtype=torch.uint8 if u8_out else torch.float32, device=dev)
    check(lib.mae_mix_batch(ptr(images), _lib.MAE_U8 if images.dtype == torch.uint8 else _lib.MAE_F32, ptr(partner), ptr(lam), ptr(box), B, C, S,
                            _lib.MAE_U8 if u8_out else _lib.MAE_F32, ptr(out), _stream(dev)))
    own = torch.arange(B, dtype=torch.int64, device=dev)
    idx = partner.to(torch.int64)
    yb = labels[torch.where((idx < 0) | (idx >= B), own, idx)]  # the kernel's rule: an out-of-range partner is the image itself
    return out, labels, yb, lam


def drop_path_rates(depth: int, rate: float) -> np.ndarray:
    """Per-block drop rates of timm's VisionTransformer: ``torch.linspace(0, rate, depth)``, p_i = rate * i / (depth - 1) (depth 1: 0)."""
    rate = float(rate)
    if not 0.0 <= rate < 1.0:
        raise ValueError(f"drop_path rate must be in [0, 1), got {rate}")
    if depth < 1:
        raise ValueError(f"depth must be positive, got {depth}")
    return np.array([rate * i / (depth - 1) if depth > 1 else 0.0 for i in range(depth)], dtype=np.float64)


def draw_drop_path(depth: int, batch: int, rate: float, gen_or_seed: Union[np.random.Generator, int, Sequence[int]]) -> torch.Tensor:
    """One step's stochastic-depth draw (timm ``DropPath``, scale_by_keep=True) as the engine's branch-scale table: a
    (2 * depth, batch) fp32 host tensor, row 2i the attention branch of block i and row 2i + 1 its MLP branch, each image kept
    independently where u >= p_i with u = default_rng(entropy).random((2 * depth, batch)).  Values are 0 (dropped) or
    float32(1 / (1 - p_i)) (kept); rows with p_i == 0 are exactly 1.  ``gen_or_seed`` as in ``draw_mix_params``.  Host arithmetic
    only: nothing here touches the device."""
    p = drop_path_rates(depth, rate)
    rng = gen_or_seed if isinstance(gen_or_seed, np.random.Generator) else np.random.default_rng(gen_or_seed)
    u = rng.random((2 * int(depth), int(batch)))
    p_rows = np.repeat(p, 2)[:, None]
    kept = (1.0 / (1.0 - p_rows)).astype(np.float32)
    return torch.from_numpy(np.where(u >= p_rows, kept, np.float32(0.0)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# per-image augmentation for fine-tuning (MAE main_finetune.py / timm create_transform: RandomResizedCrop + flip,
# RandAugment rand-m9-mstd0.5-inc1, RandomErasing p 0.25 in `pixel` mode), applied by the kernel behind mae_augment_ops_u8
# ---------------------------------------------------------------------------------------------------------------------
RAND_AUGMENT_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
                    "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")   # timm's _RAND_INCREASING_TRANSFORMS
AUG_MAX_OPS = 8   # slots of one kernel call, the crop's included


class AugParams(NamedTuple):
    """One batch's draw, host tensors: ``op_codes`` (B, K, 2) int32 (op id, integer argument) and ``op_args`` (B, K, 6) fp64
    (blend factor in [0], or the affine matrix) with slot 0 the crop + flip and slots 1.. RandAugment; ``erase`` (B, 5) int32
    (y0, y1, x0, x1, seed; an empty box = not erased), None when the configuration erases nothing (probability 0); ``crop``
    (B, 5) int32 (top, left, h, w, flip), the boxes slot 0 was made from."""
    op_codes: torch.Tensor
    op_args: torch.Tensor
    erase: Optional[torch.Tensor]
    crop: torch.Tensor


def _fill_word(fill) -> int:
    r, g, b = (int(v) for v in ((fill,) * 3 if isinstance(fill, (int, float)) else fill))
    if not all(0 <= v <= 255 for v in (r, g, b)):
        raise ValueError(f"fill must be bytes, got {fill}")
    return (r << 16) | (g << 8) | b


def affine_arg(mode: int, fill=(128, 128, 128)) -> int:
    """The integer argument of an AFFINE op, mode | fill << 8 with fill = 0xRRGGBB, as the int32 that holds those bits."""
    v = (int(mode) & 0xff) | (_fill_word(fill) << 8)
    return v - (1 << 32) if v >= 1 << 31 else v


def rotate_matrix(deg: float, size: int) -> Tuple[float, ...]:
    """The matrix ``Image.rotate(deg)`` hands to ``transform(AFFINE)``: cos / sin of -radians(deg) rounded to 15 places, the
    centre (size / 2, size / 2) carried through."""
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    c = size / 2.0
    m[2] = m[0] * -c + m[1] * -c + m[2]
    m[5] = m[3] * -c + m[4] * -c + m[5]
    m[2] += c
    m[5] += c
    return tuple(m)


def crop_matrix(top: int, left: int, h: int, w: int, flip: bool, size: int) -> Tuple[float, ...]:
    """The crop box resampled to the full frame as an affine map of output pixel centres (columns mirrored when flipped)."""
    if flip:
        return (-w / size, 0.0, float(left + w), 0.0, h / size, float(top))
    return (w / size, 0.0, float(left), 0.0, h / size, float(top))


def rand_augment_slots(which: np.ndarray, applied: np.ndarray, level: np.ndarray, positive: np.ndarray, size: int, fill=(128, 128, 128)):
    """timm's level functions of the "increasing" transforms for arrays of draws of one shape (``which`` indexes
    ``RAND_AUGMENT_OPS``, ``level`` in [0, 10]): (..., 2) int32 op ids / integer arguments and (..., 6) fp64 arguments, NONE where
    ``applied`` is False.  With s = +-1: Rotate s 30 level / 10 degrees; ShearX / ShearY s 0.3 level / 10; TranslateXRel /
    TranslateYRel s 0.45 level / 10 * size pixels; Posterize 4 - int(4 level / 10) bits; Solarize threshold 256 - int(256 level / 10);
    SolarizeAdd min(128, int(110 level / 10)); Color / Contrast / Brightness / Sharpness factor max(0.1, 1 + s 0.9 level / 10).
    Geometric ops resample bicubically (PIL's rounding) and fill with ``fill``.  Only the rotations, whose matrix goes through
    Python's ``round``, are computed one by one."""
    from . import _lib as L
    idx = {n: i for i, n in enumerate(RAND_AUGMENT_OPS)}
    codes = np.zeros(which.shape + (2,), dtype=np.int32)
    args = np.zeros(which.shape + (6,), dtype=np.float64)
    sign = np.where(positive, 1.0, -1.0)
    geo = affine_arg(L.AUG_BICUBIC, fill)
    def put(name, code, iarg=0):
        m = applied & (which == idx[name])
        codes[m, 0] = code
        codes[m, 1] = iarg[m] if isinstance(iarg, np.ndarray) else iarg
        return m
    put("AutoContrast", L.AUG_AUTOCONTRAST); put("Equalize", L.AUG_EQUALIZE); put("Invert", L.AUG_INVERT)
    put("Posterize", L.AUG_POSTERIZE, 4 - (4 * level / 10.0).astype(np.int64))
    put("Solarize", L.AUG_SOLARIZE, 256 - (256 * level / 10.0).astype(np.int64))
    put("SolarizeAdd", L.AUG_SOLARIZE_ADD, np.minimum(128, (110 * level / 10.0).astype(np.int64)))
    factor = np.maximum(0.1, 1.0 + sign * 0.9 * level / 10.0)
    for name, code in (("Color", L.AUG_COLOR), ("Contrast", L.AUG_CONTRAST), ("Brightness", L.AUG_BRIGHTNESS), ("Sharpness", L.AUG_SHARPNESS)):
        m = put(name, code)
        args[m, 0] = factor[m]
    shear, shift = sign * 0.3 * level / 10.0, sign * 0.45 * level / 10.0 * size
    for name, slot, value in (("ShearX", 1, shear), ("ShearY", 3, shear), ("TranslateXRel", 2, shift), ("TranslateYRel", 5, shift)):
        m = put(name, L.AUG_AFFINE, geo)
        args[m, 0] = 1.0; args[m, 4] = 1.0
        args[m, slot] = value[m]
    m = put("Rotate", L.AUG_AFFINE, geo)
    for i in zip(*np.nonzero(m)):
        args[i] = rotate_matrix(float(sign[i]) * 30.0 * float(level[i]) / 10.0, size)
    return codes, args


def rand_augment_op(name: str, level: float, positive: bool, size: int, fill=(128, 128, 128)):
    """One RandAugment transform of the "increasing" set at ``level`` in [0, 10] as (op id, integer argument, six fp64 arguments):
    one entry of ``rand_augment_slots``."""
    if name not in RAND_AUGMENT_OPS:
        raise ValueError(f"unknown RandAugment op {name!r}")
    codes, args = rand_augment_slots(np.array([RAND_AUGMENT_OPS.index(name)]), np.array([True]), np.array([float(level)]),
                                     np.array([bool(positive)]), size, fill)
    return int(codes[0, 0]), int(codes[0, 1]), tuple(float(v) for v in args[0])


def draw_finetune_augment(batch: int, size: int, gen_or_seed: Union[np.random.Generator, int, Sequence[int]],
                          crop_scale: Optional[Sequence[float]] = (0.08, 1.0), crop_ratio: Sequence[float] = (3.0 / 4.0, 4.0 / 3.0),
                          flip: float = 0.5, interpolation: str = "bicubic", num_ops: int = 2, magnitude: float = 9.0, mstd: float = 0.5,
                          op_prob: float = 0.5, erase_prob: float = 0.25, erase_area: Sequence[float] = (0.02, 1.0 / 3.0),
                          erase_aspect: Sequence[float] = (0.3, 1.0 / 0.3), fill=(128, 128, 128)) -> AugParams:
    """One batch's per-image augmentation draw.  Per image:
      crop   torchvision ``RandomResizedCrop.get_params``: up to ten draws of (area in ``crop_scale`` of the image, log-uniform
             aspect in ``crop_ratio``), w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)); the first with
             0 < w, h <= size is kept with a uniform integer top / left, else the whole image.  ``crop_scale`` None: no crop.
      flip   with probability ``flip``.  The box is resampled by ``interpolation`` ("bicubic" | "bilinear"), rounded to nearest.
      RandAugment  ``num_ops`` transforms drawn uniformly with replacement from ``RAND_AUGMENT_OPS``, each applied with
             probability ``op_prob`` (else NONE) at level clip(N(magnitude, mstd), 0, 10) with a fair random sign
             (``rand_augment_op``).
      erase  timm ``RandomErasing``: with probability ``erase_prob`` up to ten draws of (area in ``erase_area`` of the image,
             log-uniform aspect in ``erase_aspect``), h = round(sqrt(area * aspect)), w = round(sqrt(area / aspect)); the first
             with h < size and w < size is kept with top in [0, size - h], left in [0, size - w], and one int32 noise seed.
    ``gen_or_seed`` as in ``draw_mix_params``: the same entropy gives the same draw.  Host arithmetic only."""
    from . import _lib as L
    rng = gen_or_seed if isinstance(gen_or_seed, np.random.Generator) else np.random.default_rng(gen_or_seed)
    B, S, K = int(batch), int(size), int(num_ops)
    if interpolation not in ("bicubic", "bilinear"):
        raise ValueError(f"interpolation must be 'bicubic' or 'bilinear', got {interpolation!r}")
    if not 0 <= K <= AUG_MAX_OPS - 1:
        raise ValueError(f"num_ops must be in 0..{AUG_MAX_OPS - 1}, got {K}")
    if not all(0.0 <= p <= 1.0 for p in (flip, op_prob, erase_prob)):
        raise ValueError("flip / op_prob / erase_prob are probabilities")
    codes = np.zeros((B, 1 + K, 2), dtype=np.int32)
    args = np.zeros((B, 1 + K, 6), dtype=np.float64)
    rows = np.arange(B)

    # crop box + flip -> slot 0
    top = np.zeros(B, dtype=np.int64); left = np.zeros(B, dtype=np.int64)
    h = np.full(B, S, dtype=np.int64); w = np.full(B, S, dtype=np.int64)
    if crop_scale is not None:
        lo, hi = float(crop_scale[0]), float(crop_scale[1])
        if not 0.0 < lo <= hi:
            raise ValueError(f"crop_scale must satisfy 0 < lo <= hi, got {tuple(crop_scale)}")
        area = S * S * rng.uniform(lo, hi, (B, 10))
        ar = np.exp(rng.uniform(math.log(crop_ratio[0]), math.log(crop_ratio[1]), (B, 10)))
        cw = np.round(np.sqrt(area * ar)).astype(np.int64)
        ch = np.round(np.sqrt(area / ar)).astype(np.int64)
        ok = (cw > 0) & (cw <= S) & (ch > 0) & (ch <= S)
        first = np.argmax(ok, axis=1)
        found = ok.any(axis=1)
        w = np.where(found, cw[rows, first], S); h = np.where(found, ch[rows, first], S)
        top = np.floor(rng.random(B) * (S - h + 1)).astype(np.int64)    # randint(0, size - h + 1)
        left = np.floor(rng.random(B) * (S - w + 1)).astype(np.int64)
    flipped = rng.random(B) < flip
    moved = flipped | (h != S) | (w != S)   # the identity box without a flip is the image: nothing to run
    mode = L.AUG_BICUBIC_ROUND if interpolation == "bicubic" else L.AUG_BILINEAR_ROUND
    codes[:, 0, 0] = np.where(moved, L.AUG_AFFINE, L.AUG_NONE)
    codes[:, 0, 1] = np.where(moved, affine_arg(mode, fill), 0)
    sx = w / S
    args[:, 0, 0] = np.where(flipped, -sx, sx); args[:, 0, 2] = np.where(flipped, left + w, left).astype(np.float64)
    args[:, 0, 4] = h / S; args[:, 0, 5] = top.astype(np.float64)
    args[~moved, 0] = 0.0

    # RandAugment -> slots 1..K
    if K > 0:
        which = rng.integers(0, len(RAND_AUGMENT_OPS), (B, K))
        applied = rng.random((B, K)) < op_prob
        level = np.clip(rng.normal(magnitude, mstd, (B, K)) if mstd > 0 else np.full((B, K), float(magnitude)), 0.0, 10.0)
        positive = rng.random((B, K)) < 0.5
        codes[:, 1:], args[:, 1:] = rand_augment_slots(which, applied, level, positive, S, fill)

    # random erasing
    erase = None
    if erase_prob > 0.0:
        erase = np.zeros((B, 5), dtype=np.int32)
        chosen = rng.random(B) < erase_prob
        area = S * S * rng.uniform(erase_area[0], erase_area[1], (B, 10))
        ar = np.exp(rng.uniform(math.log(erase_aspect[0]), math.log(erase_aspect[1]), (B, 10)))
        eh = np.round(np.sqrt(area * ar)).astype(np.int64)
        ew = np.round(np.sqrt(area / ar)).astype(np.int64)
        ok = (eh < S) & (ew < S) & (eh > 0) & (ew > 0)
        first = np.argmax(ok, axis=1)
        found = ok.any(axis=1) & chosen
        eh, ew = eh[rows, first], ew[rows, first]
        y0 = np.floor(rng.random(B) * (S - eh + 1)).astype(np.int64)    # randint(0, size - h), both ends included
        x0 = np.floor(rng.random(B) * (S - ew + 1)).astype(np.int64)
        seeds = rng.integers(-2 ** 31, 2 ** 31, B)
        erase[:, 0] = np.where(found, y0, 0); erase[:, 1] = np.where(found, y0 + eh, 0)
        erase[:, 2] = np.where(found, x0, 0); erase[:, 3] = np.where(found, x0 + ew, 0)
        erase[:, 4] = np.where(found, seeds, 0)
    crop = np.stack([top, left, h, w, flipped.astype(np.int64)], axis=1).astype(np.int32)
    return AugParams(op_codes=torch.from_numpy(codes), op_args=torch.from_numpy(args),
                     erase=None if erase is None else torch.from_numpy(erase), crop=torch.from_numpy(crop))


def augment_finetune(images: torch.Tensor, params: AugParams, out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """A uint8 device batch through its draw, by the HIP kernel behind ``mae_augment_ops_u8``: the ops of every image in slot
    order, then -- with fp32 output -- normalisation and the erase noise.  Returns uint8 when the configuration erases nothing
    (``params.erase`` is None), so that the batch stays 1 byte per pixel, and normalised fp32 otherwise; ``out_dtype``
    overrides, except that erasing needs fp32 (normal noise has no byte form).  The draw reaches the device through pinned
    memory: no host-device synchronisation.  No torch fallback."""
    from . import _lib
    from ._lib import check, lib, ptr
    from .mae import _stream
    if images.dtype != torch.uint8 or not images.is_cuda or images.dim() != 4 or images.shape[2] != images.shape[3]:
        raise ValueError(f"augment_finetune needs a square (B, C, S, S) uint8 CUDA batch, got {tuple(images.shape)} {images.dtype} on {images.device}")
    B, C, S, _ = images.shape
    K = params.op_codes.shape[1] if params.op_codes.dim() == 3 else -1
    if params.op_codes.shape != (B, K, 2) or params.op_args.shape != (B, K, 6) or (params.erase is not None and params.erase.shape != (B, 5)):
        raise ValueError(f"augment_finetune: the parameters are not those of a batch of {B}")
    if out_dtype is None:
        out_dtype = torch.uint8 if params.erase is None else torch.float32
    if out_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"augment_finetune: out_dtype must be uint8 or float32, got {out_dtype}")
    if params.erase is not None and out_dtype == torch.uint8:
        raise ValueError("augment_finetune: random erasing writes normal noise in normalised space and needs float32 output")
    dev = images.device
    def up(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:  # a draw already on the device passes through
        t = t.to(dt).contiguous()
        return t.to(dev) if t.is_cuda else t.pin_memory().to(dev, non_blocking=True)
    flags = _lib.MAE_U8 if out_dtype == torch.uint8 else _lib.MAE_F32
    if C != 3 and K > 0 and not params.op_codes.is_cuda:
        ids = params.op_codes[:, :, 0]
        if bool(((ids == _lib.AUG_NONE) | (ids == _lib.AUG_AFFINE)).all()):
            flags |= _lib.AUG_GEOMETRIC   # stated only where it is true: anything else is refused by the launcher
    codes = up(params.op_codes, torch.int32) if K > 0 else None
    args = up(params.op_args, torch.float64) if K > 0 else None
    erase = up(params.erase, torch.int32) if params.erase is not None else None
    images = images.contiguous()
    out = torch.empty((B, C, S, S), dtype=out_dtype, device=dev)
    check(lib.mae_augment_ops_u8(ptr(images), B, C, S, ptr(codes), ptr(args), K, ptr(erase), flags, ptr(out), _stream(dev)))
    return out
