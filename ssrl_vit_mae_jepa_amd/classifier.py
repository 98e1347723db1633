"""The downstream classifier of the reference (``src/models/classifier.py``, ``src/training/classifier.py``) on the engine.

``ViTClassifier`` wraps the engine's encoder node (``mae.encoder.vit``, what ``scripts/training/train_mae.py:143`` hands
the reference's classifier) and a ``ClassificationHead`` whose ``weight`` / ``bias`` live in one flat fp32 buffer (W then
b, the layout the C ABI reads).  ``ViTClassifierTrainModule`` keeps the reference's keys, defaults, freeze methods and
logged names, and adds the native step: one call for forward + pooled head + cross-entropy + a backward that stops where
the trainable blocks end, then clip_grad_norm_(1.0) + one-group AdamW over exactly the tensors whose ``requires_grad``
is set (Lightning ``gradient_clip_val=1.0``, scripts/training/train_mae.py:213; src/training/classifier.py:106-108).

The native calls are the widest entry points of the C ABI (``mae_engine_classifier_forward_ex``, ``..._loss_and_grads_sd``), whatever
the configuration: an option that is off is an argument left at None / 0, and the engine then issues the launches -- and the bits -- of
the narrower entry points.

The fine-tuning recipe of the MAE paper (not in the reference; every option off by default): ``train.label_smoothing``, ``train.mixup_alpha`` / ``train.cutmix_alpha`` (+ ``mix_prob``, ``mix_switch_prob``)
mix each training batch on the device (``data.mix_batch``) and train on the soft targets inside the head kernel;
``train.layer_decay`` scales the learning rate of layer l by ``layer_decay ** (depth + 1 - l)`` (BEiT / MAE numbering);
``train.augment`` augments each image of a training batch before all that (``data.augment_finetune``: RandomResizedCrop + flip,
RandAugment, random erasing, one kernel).  With a model of another size than the dataset the order is: the ops at the dataset's
resolution, then the resize to ``image_size`` (``data.resize_batch``), then mixup / CutMix at the model's size.
"""
from __future__ import annotations

import ctypes as C
import math
import sys
from typing import Any, Dict, List, Optional, Tuple

import torch
from torch import nn

from . import _lib
from ._lib import check, lib
from .mae import MaskedAutoencoder, _ptr, _stream, _ViT
from .training import AccumulationWindow, lr_lambda

POOLS = {"cls": _lib.POOL_CLS, "mean": _lib.POOL_MEAN, "mean_patches": _lib.POOL_MEAN_PATCHES}
NO_CLS_POOL = "pool 'cls' needs a class token: I-JEPA encoders are trained on the patch tokens only (use 'mean' or 'mean_patches')"
MAX_CLASSES = 128


def _pad4(n: int) -> int:
    return (n + 3) // 4 * 4


class ClassificationHead(nn.Module):
    """src/models/classifier.py:10-22: ``.classification`` = Linear(input_dim, output_dim), initialised as nn.Linear is.
    Its weight and bias are views into ``flat`` (W then b, padded to a multiple of 4 floats)."""

    def __init__(self, input_dim: int, output_dim: int) -> None:
        super().__init__()
        self.input_dim, self.output_dim = int(input_dim), int(output_dim)
        self.classification = nn.Linear(self.input_dim, self.output_dim)
        self.flat = torch.zeros(_pad4(self.output_dim * self.input_dim + self.output_dim), dtype=torch.float32)
        self._reflatten(self.flat.device)

    @property
    def numel(self) -> int:
        return self.output_dim * self.input_dim + self.output_dim

    @torch.no_grad()
    def _reflatten(self, device: torch.device) -> None:
        w, b = self.classification.weight, self.classification.bias
        nw = w.numel()
        if self.flat.device != device:
            self.flat = torch.zeros(self.flat.numel(), dtype=torch.float32, device=device)
        for p, lo, n in ((w, 0, nw), (b, nw, b.numel())):
            view = self.flat[lo:lo + n].view(p.shape)
            if p.data.data_ptr() != view.data_ptr():
                view.copy_(p.data.to(device=device, dtype=torch.float32))
                p.data = view
                p.grad = None

    def _apply(self, fn, recurse=True):
        super()._apply(fn)
        self._reflatten(self.classification.weight.device)
        return self

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.classification(x)


class ViTClassifier(nn.Module):
    """src/models/classifier.py:25-57 over the engine: ``encoder`` is the engine's ``_ViT`` node, ``head`` the linear head,
    ``pool_type`` "cls", "mean" (every row of the sequence) or "mean_patches" (the patch rows: timm's global_pool="avg").
    ``forward`` is an inference call (the training route is the native step of ``ViTClassifierTrainModule``).

    The sequence follows the encoder node's ``with_cls``: True is [cls | patches]; False (an encoder loaded by
    ``representation.load_ijepa_encoder``) is the patch tokens alone, where "mean" and "mean_patches" are the same pool and
    "cls" is refused."""

    def __init__(self, pretrained_encoder: _ViT, num_classes: int = 10, head_cfg: Optional[Dict[str, Any]] = None):
        super().__init__()
        if not isinstance(pretrained_encoder, _ViT):
            raise TypeError("ViTClassifier needs the engine's encoder node (MaskedAutoencoder(...).encoder.vit)")
        head_cfg = head_cfg or {}
        embed_dim = int(head_cfg.get("embed_dim", pretrained_encoder.embed_dim))
        if embed_dim != pretrained_encoder.embed_dim:
            raise ValueError(f"head embed_dim {embed_dim} != encoder width {pretrained_encoder.embed_dim}")
        pool_type = head_cfg.get("pool", "cls")
        if pool_type not in POOLS:
            raise ValueError(f"pool must be 'cls', 'mean' or 'mean_patches', got {pool_type!r}")
        if pool_type == "cls" and not pretrained_encoder.with_cls:
            raise ValueError(NO_CLS_POOL)
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [2, {MAX_CLASSES}], got {num_classes}")
        self.encoder = pretrained_encoder
        self.pool_type = pool_type
        self.num_classes = int(num_classes)
        self.head = ClassificationHead(input_dim=embed_dim, output_dim=self.num_classes)

    @property
    def mae(self) -> MaskedAutoencoder:
        return self.encoder._owner()

    @property
    def with_cls(self) -> bool:
        return bool(self.encoder.with_cls)

    @property
    def extended(self) -> bool:
        """True for a patch-only sequence or the patch-row mean: what the first-generation entry points of the C ABI
        (``with_cls = 1``, "cls" or "mean") cannot express.  Such a head pools through the row-range kernel."""
        return not self.with_cls or self.pool_type == "mean_patches"

    def _apply(self, fn, recurse=True):
        # the encoder's tensors are views into the MAE's arena: move them through their owner, which re-flattens them
        self.mae._apply(fn)
        self.head._apply(fn)
        return self

    def workspace(self, batch: int) -> torch.Tensor:
        """The owner's workspace grown to the classifier's size.  It is shared with the MAE's forwards, so every saved
        activation of an earlier call is invalidated: a pending hand-off backward refuses to run."""
        m = self.mae
        need = lib.mae_engine_classifier_workspace_bytes_ex(m.engine.handle, batch, self.num_classes, int(self.with_cls))
        if need < 0:
            raise ValueError(f"bad batch {batch} / num_classes {self.num_classes}")
        if m._workspace is None or m._workspace.numel() < need or m._workspace.device != m.flat_params.device:
            m._workspace = None
            m._workspace = torch.empty(need, dtype=torch.uint8, device=m.flat_params.device)
        m._gen_enc += 1; m._gen_dec += 1
        m._plan = None
        return m._workspace

    def _guard(self) -> None:
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("ViTClassifier.forward() is an inference call on the MI355X engine and records no autograd graph; "
                               "train through ViTClassifierTrainModule.loss_and_grads()/fused_training_step(), or wrap the call "
                               "in torch.no_grad()")

    def evaluate(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None, logits: bool = True):
        """Native forward: returns (logits or None, loss or None, correct count or None), device tensors."""
        m = self.mae
        dev = m._require_cuda()
        images = m._check_images(images)
        B = images.shape[0]
        out = torch.empty(B, self.num_classes, dtype=torch.float32, device=dev) if logits else None
        loss = correct = None
        if labels is not None:
            labels = labels.to(device=dev, dtype=torch.int64).contiguous()
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            correct = torch.empty(1, dtype=torch.int32, device=dev)
        ws = self.workspace(B)
        check(lib.mae_engine_classifier_forward_ex(
            m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(self.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B,
            int(self.with_cls), POOLS[self.pool_type], self.num_classes, _ptr(ws), ws.numel(), _ptr(out), _ptr(loss), _ptr(correct), _stream(dev)))
        return out, loss, correct

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._guard()
        return self.evaluate(x)[0]


def parse_augment(block: Optional[Dict[str, Any]]) -> Optional[Dict[str, Any]]:
    """``train.augment`` checked and turned into the keyword arguments of ``data.draw_finetune_augment``; None when the block is
    absent or empty.  Keys: ``crop_scale`` [lo, hi] (absent: no crop), ``flip`` (probability, absent: 0), ``interpolation``
    (bicubic | bilinear), ``rand_augment`` {num_ops, magnitude, mstd, prob} (absent: no ops), ``random_erasing`` (probability,
    absent: 0), ``fill`` (a byte, or three).  The ops run at the resolution the training batch arrives in: for a model of another
    size than the dataset that is the dataset's (``get_train_batches(train_at_dataset_size=True)``), and the resize to the model's size
    follows them -- uint8 -> uint8 / fp32 without erasing, fp32 -> fp32 with it -- before mixup / CutMix."""
    if not block:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"train.augment must be a mapping, got {block!r}")
    unknown = set(block) - {"crop_scale", "flip", "interpolation", "rand_augment", "random_erasing", "fill"}
    if unknown:
        raise ValueError(f"train.augment: unknown keys {sorted(unknown)}")
    crop = block.get("crop_scale")
    if crop is not None:
        if not isinstance(crop, (list, tuple)) or len(crop) != 2 or not 0.0 < float(crop[0]) <= float(crop[1]) <= 1.0:
            raise ValueError(f"train.augment.crop_scale must be [lo, hi] with 0 < lo <= hi <= 1, got {crop!r}")
        crop = (float(crop[0]), float(crop[1]))
    flip, erase = float(block.get("flip", 0.0) or 0.0), float(block.get("random_erasing", 0.0) or 0.0)
    if not (0.0 <= flip <= 1.0 and 0.0 <= erase <= 1.0):
        raise ValueError(f"train.augment.flip / random_erasing are probabilities, got {flip} / {erase}")
    interpolation = block.get("interpolation", "bicubic")
    if interpolation not in ("bicubic", "bilinear"):
        raise ValueError(f"train.augment.interpolation must be bicubic or bilinear, got {interpolation!r}")
    ra = block.get("rand_augment")
    if ra is not None and not isinstance(ra, dict):
        raise ValueError(f"train.augment.rand_augment must be a mapping, got {ra!r}")
    if ra is not None and set(ra) - {"num_ops", "magnitude", "mstd", "prob"}:
        raise ValueError(f"train.augment.rand_augment: unknown keys {sorted(set(ra) - {'num_ops', 'magnitude', 'mstd', 'prob'})}")
    num_ops = int(ra.get("num_ops", 2)) if ra is not None else 0
    magnitude, mstd, prob = (float((ra or {}).get(k, d)) for k, d in (("magnitude", 9.0), ("mstd", 0.5), ("prob", 0.5)))
    if not (0 <= num_ops <= 7 and 0.0 <= magnitude <= 10.0 and mstd >= 0.0 and 0.0 <= prob <= 1.0):
        raise ValueError("train.augment.rand_augment: num_ops in 0..7, magnitude in [0, 10], mstd >= 0, prob in [0, 1]")
    fill = block.get("fill", 128)
    fill = tuple(fill) if isinstance(fill, (list, tuple)) else (fill,) * 3
    if len(fill) != 3 or not all(isinstance(v, int) and 0 <= v <= 255 for v in fill):
        raise ValueError(f"train.augment.fill must be a byte or three, got {block.get('fill')!r}")
    return dict(crop_scale=crop, flip=flip, interpolation=interpolation, num_ops=num_ops, magnitude=magnitude, mstd=mstd, op_prob=prob,
                erase_prob=erase, fill=fill)


def _group_of(name: str) -> str:
    if name.startswith("blocks."):
        return "blocks." + name.split(".")[1]
    if name.startswith("norm."):
        return "norm"
    return "embed"  # cls_token, pos_embed, patch_embed.proj.*


class ViTClassifierTrainModule(nn.Module):
    """src/training/classifier.py:16-171 without Lightning, plus the native fused step."""

    def __init__(self, pretrained_encoder: Optional[_ViT] = None, model_cfg: Optional[Dict[str, Any]] = None,
                 training_cfg: Optional[Dict[str, Any]] = None, num_classes: int = 10):
        super().__init__()
        self.model_cfg = model_cfg or {}
        self.training_cfg = training_cfg or {}
        self.hparams = {"model_cfg": self.model_cfg, "training_cfg": self.training_cfg, "num_classes": num_classes}
        self.learning_rate = float(self.training_cfg.get("learning_rate", 3e-4))
        self.weight_decay = float(self.training_cfg.get("weight_decay", 0.05))
        self.warmup_epochs = int(self.training_cfg.get("warmup_epochs", 5))
        self.total_epochs = int(self.training_cfg.get("total_epochs", 100))
        self.freeze_encoder_flag = self.training_cfg.get("freeze_encoder", True)
        self.num_classes = num_classes
        self.gradient_clip_val = 1.0
        self.label_smoothing = float(self.training_cfg.get("label_smoothing", 0.0) or 0.0)
        self.mixup_alpha = float(self.training_cfg.get("mixup_alpha", 0.0) or 0.0)
        self.cutmix_alpha = float(self.training_cfg.get("cutmix_alpha", 0.0) or 0.0)
        self.mix_prob = float(self.training_cfg.get("mix_prob", 1.0))
        self.mix_switch_prob = float(self.training_cfg.get("mix_switch_prob", 0.5))
        self.layer_decay = float(self.training_cfg.get("layer_decay", 1.0))
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"train.label_smoothing must be in [0, 1), got {self.label_smoothing}")
        if self.mixup_alpha < 0 or self.cutmix_alpha < 0 or not 0.0 < self.layer_decay <= 1.0:
            raise ValueError("train.mixup_alpha / cutmix_alpha must be >= 0 and train.layer_decay in (0, 1]")
        if not (0.0 <= self.mix_prob <= 1.0 and 0.0 <= self.mix_switch_prob <= 1.0):
            raise ValueError(f"train.mix_prob / mix_switch_prob must be in [0, 1], got {self.mix_prob} / {self.mix_switch_prob}")
        self.drop_path = float(self.training_cfg.get("drop_path", 0.0) or 0.0)
        if not 0.0 <= self.drop_path < 1.0:
            raise ValueError(f"train.drop_path must be in [0, 1), got {self.drop_path}")
        self.augment = parse_augment(self.training_cfg.get("augment"))
        general = self.model_cfg.get("general") or {}
        if self.augment is not None and "image_size" in general:
            from .data import DATASET_SIZE
            ops_size = min(int(general["image_size"]), DATASET_SIZE)  # a larger model is fed through the resize: the ops run on the dataset's own pixels
            need = 2 * int(general.get("in_chans", 3)) * ops_size ** 2 + 3200
            if need > 160 * 1024:
                raise ValueError(f"train.augment keeps two copies of an image in LDS: {need} bytes at image size {ops_size}, more than 160 KiB")
        self.aug_seed = 73
        self._aug_step = 0
        self.mix_seed = 73
        self._mix_step = 0
        self.drop_seed = 73
        self._drop_step = 0
        self._drop_ignored_said = False
        self.accumulate_grad_batches = int(self.training_cfg.get("accumulate_grad_batches", 1))  # micro-batches per optimizer step; learning_rate stays absolute
        if self.accumulate_grad_batches < 1:
            raise ValueError(f"train.accumulate_grad_batches must be at least 1, got {self.accumulate_grad_batches}")
        self._window = AccumulationWindow()
        self._stashes: Dict[str, torch.Tensor] = {}
        self.current_epoch = 0
        self.logged: Dict[str, Any] = {}
        encoder = pretrained_encoder if pretrained_encoder is not None else build_baseline_encoder(self.model_cfg)
        self.model = ViTClassifier(pretrained_encoder=encoder, num_classes=self.num_classes, head_cfg=self.model_cfg.get("head", {}))
        self._opt: Dict[str, torch.Tensor] = {}
        self._opt_steps = 0
        self._pos_grad: Optional[torch.Tensor] = None
        self._head_grad: Optional[torch.Tensor] = None
        if self.freeze_encoder_flag:
            self.freeze_encoder()
        else:
            self.unfreeze_encoder()

    # ---- reference surface ---------------------------------------------------------------------
    def forward(self, x: torch.Tensor):
        return self.model(x)

    def log(self, name: str, value, **_kw) -> None:
        self.logged[name] = value  # device tensors stay on device: no host sync in the step

    def freeze_encoder(self):
        for name, param in self.model.named_parameters():
            if "head" not in name:
                param.requires_grad = False

    def unfreeze_encoder(self):
        for param in self.model.parameters():
            param.requires_grad = True

    def unfreeze_last_layers(self, n_layers: int):
        encoder = self.model.encoder
        blocks = encoder.blocks
        total = len(blocks)
        if n_layers < 0 or n_layers > total:
            raise ValueError(f"n_layers must be between 0 and {total}, got {n_layers}")
        for param in encoder.parameters():
            param.requires_grad = False
        for block in blocks[total - n_layers:]:
            for param in block.parameters():
                param.requires_grad = True
        if hasattr(encoder, "norm"):
            for param in encoder.norm.parameters():
                param.requires_grad = True
        for param in self.model.head.parameters():
            param.requires_grad = True

    def current_lr(self, epoch: Optional[int] = None) -> float:
        """LambdaLR per epoch over learning_rate (src/training/classifier.py:113-119); no batch-size scaling."""
        return self.learning_rate * lr_lambda(self.current_epoch if epoch is None else epoch, self.warmup_epochs, self.total_epochs)

    def _eval_step(self, batch, prefix: str):
        imgs, labels = batch
        with torch.no_grad():
            _logits, loss, correct = self.model.evaluate(imgs, labels, logits=False)
        self.log(f"{prefix}_loss", loss[0])
        self.log(f"{prefix}_acc", correct[0].float() / imgs.shape[0])
        return loss[0]

    def training_step(self, batch, batch_idx):
        """Loss + gradients of the trainable set (native); ``optimizer_step`` applies them."""
        imgs, labels = batch
        imgs = self._augment(imgs)
        loss, correct = self.loss_and_grads(imgs, labels, branch_scale=self._draw_branch_scale(imgs.shape[0]))
        self.log("train_loss", loss[0])
        self.log("train_acc", correct[0].float() / imgs.shape[0])
        return loss[0]

    def validation_step(self, batch, batch_idx):
        return self._eval_step(batch, "val")

    def test_step(self, batch, batch_idx):
        return self._eval_step(batch, "test")

    # ---- trainable set ---------------------------------------------------------------------------
    def train_mode(self) -> Tuple[int, int]:
        """(train_blocks, train_embed) of the C ABI from the requires_grad flags; a pattern the native backward cannot
        express raises ValueError naming the tensors (it never trains another set than the flags describe)."""
        enc = self.model.encoder
        depth = len(enc.blocks)
        groups: Dict[str, List[Tuple[str, bool]]] = {}
        for name, p in enc.named_parameters():
            groups.setdefault(_group_of(name), []).append((name, p.requires_grad))
        head_frozen = [f"head.{n}" for n, p in self.model.head.named_parameters() if not p.requires_grad]
        if head_frozen:
            raise ValueError(f"the classifier head is always trained; frozen: {head_frozen}")
        state = {}
        for g, items in groups.items():
            flags = {f for _n, f in items}
            if len(flags) > 1:
                raise ValueError(f"encoder group {g} is partly trainable: {[('encoder.' + n, f) for n, f in items]}")
            state[g] = flags.pop()
        blocks = [state[f"blocks.{i}"] for i in range(depth)]
        n = 0
        while n < depth and blocks[depth - 1 - n]:
            n += 1
        if any(blocks[: depth - n]):
            bad = [f"encoder.blocks.{i}" for i in range(depth - n) if blocks[i]]
            raise ValueError(f"trainable blocks must be a suffix of the encoder: {bad} train while encoder.blocks.{depth - n - 1} is frozen")
        if not state["norm"]:
            if n or state["embed"]:
                raise ValueError("encoder.norm.* is frozen while earlier encoder tensors train: not a trainable suffix")
            return -1, 0
        if state["embed"]:
            if n != depth:
                raise ValueError(f"encoder embedding tensors (cls_token, pos_embed, patch_embed.proj.*) train while "
                                 f"encoder.blocks.{depth - n - 1} is frozen")
            return depth, 1
        return n, 0

    def _arena_range(self, train_blocks: int, train_embed: int) -> Tuple[int, int]:
        m = self.model.mae
        hi = lib.mae_engine_encoder_grad_elems(m.engine.handle)
        if train_blocks < 0:
            return hi, hi
        if train_embed:
            return 0, hi
        depth = len(self.model.encoder.blocks)
        first = f"encoder.vit.blocks.{depth - train_blocks}.norm1.weight" if train_blocks else "encoder.vit.norm.weight"
        return m._offsets[first][1], hi

    def _update_ranges(self, train_blocks: int, train_embed: int) -> Tuple[List[Tuple[int, int]], int]:
        """What AdamW may touch: the (lo, count) pieces of the arena range and the first pos_embed row.  A patch-only
        encoder never reads cls_token or pos_embed[:, 0]; their gradients are zero, but weight decay alone would shrink
        them, so they are cut out of the update (every piece stays a multiple of 4 floats: offsets are, and so is D)."""
        lo, hi = self._arena_range(train_blocks, train_embed)
        if hi <= lo:
            return [], 0
        if not train_embed or self.model.with_cls:
            return [(lo, hi - lo)], 0
        _n, c_off, c_n, _s, _f = self.model.mae._offsets["encoder.vit.cls_token"]
        pieces = [(a, b - a) for a, b in ((lo, c_off), (c_off + c_n, hi)) if b > a]
        return pieces, 1

    def layer_of(self, name: str) -> int:
        """Layer number of an encoder tensor (timm name) or "head": embeddings 0, blocks.i -> i + 1, norm and the head
        depth + 1 (BEiT's get_num_layer_for_vit, the numbering of MAE's param_groups_lrd)."""
        depth = len(self.model.encoder.blocks)
        if name.startswith("blocks."):
            return int(name.split(".")[1]) + 1
        if name in ("cls_token", "pos_embed") or name.startswith("patch_embed."):
            return 0
        return depth + 1

    def layer_scale(self, layer: int) -> float:
        return self.layer_decay ** (len(self.model.encoder.blocks) + 1 - layer)

    def _decay_groups(self, train_blocks: int, train_embed: int) -> Tuple[List[Tuple[int, int, float]], int]:
        """``_update_ranges`` cut at the block boundaries: (lo, count, lr scale) per piece and layer.  The boundaries are tensor
        offsets, multiples of 64.  layer_decay == 1 returns the pieces of ``_update_ranges`` themselves, scale 1.0."""
        pieces, pos_row0 = self._update_ranges(train_blocks, train_embed)
        if self.layer_decay == 1.0:
            return [(lo, n, 1.0) for lo, n in pieces], pos_row0
        m = self.model.mae
        depth = len(self.model.encoder.blocks)
        starts = [m._offsets[f"encoder.vit.blocks.{i}.norm1.weight"][1] for i in range(depth)] + [m._offsets["encoder.vit.norm.weight"][1]]
        groups: List[Tuple[int, int, float]] = []
        for lo, n in pieces:
            cuts = [lo] + [c for c in starts if lo < c < lo + n] + [lo + n]
            for a, b in zip(cuts, cuts[1:]):
                layer = sum(1 for c in starts if c <= a)  # 0 below blocks.0, i + 1 inside blocks.i, depth + 1 from norm on
                groups.append((a, b - a, self.layer_scale(layer)))
        return groups, pos_row0

    # ---- native step -------------------------------------------------------------------------------
    def _grad_buffers(self):
        m = self.model.mae
        dev = m.flat_params.device
        if self._head_grad is None or self._head_grad.device != dev:
            self._head_grad = torch.zeros(self.model.head.flat.numel(), dtype=torch.float32, device=dev)
            self._pos_grad = torch.zeros(m.sequence_length * m._dims["embed_dim"], dtype=torch.float32, device=dev)
        return self._head_grad, self._pos_grad

    @property
    def head_grads(self) -> torch.Tensor:
        return self._grad_buffers()[0]

    @property
    def pos_grads(self) -> torch.Tensor:
        return self._grad_buffers()[1]

    def loss_and_grads(self, images: torch.Tensor, labels: torch.Tensor, grad_scale: float = 1.0,
                       logits_out: Optional[torch.Tensor] = None, labels_b: Optional[torch.Tensor] = None,
                       lam: Optional[torch.Tensor] = None, label_smoothing: Optional[float] = None,
                       branch_scale: Optional[torch.Tensor] = None):
        """Forward + cross-entropy + backward of the trainable set in one native call.  Gradients land in
        ``model.mae.flat_grads`` (blocks / norm / embeddings, at their arena offsets; frozen rows are not written),
        ``head_grads`` (W then b) and ``pos_grads``.  Returns device tensors (loss[1], correct[1]); no host sync.
        Soft targets: ``labels_b`` (B) and ``lam`` (B, fp32) mix the labels as lam * labels + (1 - lam) * labels_b,
        ``label_smoothing`` (None: ``train.label_smoothing``) smooths them; ``correct`` counts argmax == labels.  With none
        of the three active the engine launches the hard-label kernels.
        Drop path: ``branch_scale`` (2 * depth, B) fp32, the table ``data.draw_drop_path`` returns (row 2i: the attention branch
        of blocks.i, 2i + 1: its MLP branch), scales each image's residual branches in the forward and their gradients in the
        backward.  A host table is uploaded through pinned memory (no synchronisation); a frozen encoder refuses one."""
        tb, te = self.train_mode()
        clf, m = self.model, self.model.mae
        dev = m._require_cuda()
        images = m._check_images(images)
        B = images.shape[0]
        labels = labels.to(device=dev, dtype=torch.int64).contiguous()
        if labels.shape != (B,):
            raise ValueError(f"labels must be ({B},), got {tuple(labels.shape)}")
        head_g, pos_g = self._grad_buffers()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        correct = torch.empty(1, dtype=torch.int32, device=dev)
        ws = clf.workspace(B)
        eps = self.label_smoothing if label_smoothing is None else float(label_smoothing)
        if branch_scale is not None:
            depth = len(clf.encoder.blocks)
            if tb < 0:
                raise ValueError("branch_scale (drop path) needs a training encoder: the linear probe's encoder is in inference")
            if branch_scale.shape != (2 * depth, B):
                raise ValueError(f"branch_scale must be ({2 * depth}, {B}), got {tuple(branch_scale.shape)}")
            branch_scale = branch_scale.to(torch.float32).contiguous()
            branch_scale = branch_scale.to(dev) if branch_scale.is_cuda else branch_scale.pin_memory().to(dev, non_blocking=True)
        if labels_b is not None:
            labels_b = labels_b.to(device=dev, dtype=torch.int64).contiguous()
        if lam is not None:
            lam = lam.to(device=dev, dtype=torch.float32).contiguous()
        if any(t is not None and t.shape != (B,) for t in (labels_b, lam)):
            raise ValueError(f"labels_b and lam must be ({B},)")
        check(lib.mae_engine_classifier_loss_and_grads_sd(
            m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B,
            int(clf.with_cls), POOLS[clf.pool_type], clf.num_classes, tb, te, float(grad_scale), _ptr(ws), ws.numel(), _ptr(m.flat_grads),
            _ptr(head_g), _ptr(pos_g), _ptr(logits_out), _ptr(loss), _ptr(correct), _ptr(labels_b), _ptr(lam), eps, _ptr(branch_scale),
            _stream(dev)))
        self._last_mode = (tb, te)
        return loss, correct

    def _augment(self, images: torch.Tensor) -> torch.Tensor:
        """A training batch through ``train.augment`` (crop + flip, RandAugment, erasing: ``data.augment_finetune``), the draw a
        function of (aug_seed, current_epoch, step); the batch itself, untouched, when the key is not set.  uint8 batches only:
        the ops are those of PIL images.  A batch of another size than the model's (the dataset's own resolution, what
        ``get_train_batches(train_at_dataset_size=True)`` serves) is augmented at ITS size -- the kernel holds an image in LDS and
        takes none above 160 x 160 -- and resized to the model's afterwards (``data.resize_batch``): uint8 -> uint8, or normalised
        fp32 where the engine reads no bytes; the fp32 batch that erasing leaves -> fp32.  mixup / CutMix then see model-size images."""
        if self.augment is None:
            return images
        from .data import augment_finetune, draw_finetune_augment, resize_batch
        m = self.model.mae
        resize = images.dim() == 4 and images.shape[2] == images.shape[3] and images.shape[1] == m.in_chans and images.shape[-1] != m.image_size
        images = (images.contiguous() if resize else m._check_images(images)).to(m._require_cuda())
        if images.dtype != torch.uint8:
            raise ValueError("train.augment works on uint8 pixels (the ops are those of PIL images): serve the batch as uint8")
        params = draw_finetune_augment(images.shape[0], images.shape[-1], (self.aug_seed, self.current_epoch, self._aug_step), **self.augment)
        self._aug_step += 1
        images = augment_finetune(images, params)
        if resize:
            reads_u8 = m.patch_size % 4 == 0 and m.image_size // m.patch_size <= 64
            images = resize_batch(images, m.image_size, out_dtype=None if (reads_u8 or images.dtype != torch.uint8) else torch.float32)
        return images

    def _draw_branch_scale(self, batch: int) -> Optional[torch.Tensor]:
        """This step's drop-path table (host), a function of (drop_seed, current_epoch, step); None with rate 0.  With a frozen
        encoder (the linear probe, whose encoder is in inference) the rate is ignored, and said so once."""
        if self.drop_path <= 0.0:
            return None
        if self.train_mode()[0] < 0:
            if not self._drop_ignored_said:
                print(f"train.drop_path = {self.drop_path} is ignored: the encoder is frozen (linear probe), and a frozen encoder never drops",
                      file=sys.stderr)
                self._drop_ignored_said = True
            return None
        from .data import draw_drop_path
        table = draw_drop_path(len(self.model.encoder.blocks), batch, self.drop_path, (self.drop_seed, self.current_epoch, self._drop_step))
        self._drop_step += 1
        return table

    def _state(self, key: str, n: int, dev) -> torch.Tensor:
        t = self._opt.get(key)
        if t is None or t.device != dev or t.numel() != n:
            t = self._opt[key] = torch.zeros(n, dtype=torch.float32, device=dev)
        return t

    def optimizer_step(self, lr: Optional[float] = None) -> torch.Tensor:
        """clip_grad_norm_(gradient_clip_val) over the trainable set, then AdamW(betas (0.9, 0.999), eps 1e-8,
        weight_decay) on it, then the bf16 operand copies of the updated matrices.  Returns the device [norm, coef]."""
        tb, te = getattr(self, "_last_mode", None) or self.train_mode()
        clf, m = self.model, self.model.mae
        dev = m._require_cuda()
        h = m.engine.handle
        head_g, pos_g = self._grad_buffers()
        lo, hi = self._arena_range(tb, te)
        n_arena = m.engine.trainable_elems
        stats = self._state("stats", 8, dev)
        sums = self._state("sumsq", 4, dev)
        scratch = m._scratch_f32()
        self._opt_steps += 1
        step = self._opt_steps
        lr = float(self.current_lr() if lr is None else lr)
        hyper = (lr, 0.9, 0.999, 1e-8, float(self.weight_decay), step)
        s = _stream(dev)
        if hi > lo:
            check(lib.mae_engine_grad_sumsq_range(h, _ptr(m.flat_grads), lo, hi - lo, _ptr(sums), _ptr(scratch), s))
        check(lib.mae_engine_grad_sumsq_buffer(h, _ptr(head_g), head_g.numel(), int(hi > lo), _ptr(sums), _ptr(scratch), s))
        if te:
            check(lib.mae_engine_grad_sumsq_buffer(h, _ptr(pos_g), pos_g.numel(), 1, _ptr(sums), _ptr(scratch), s))
        check(lib.mae_engine_clip_from_sumsq(h, _ptr(sums), float(self.gradient_clip_val), _ptr(stats), s))
        pieces, pos_row0 = self._decay_groups(tb, te)  # layer_decay == 1: the pieces of _update_ranges, lr unchanged
        for p_lo, p_n, scale in pieces:
            ea, eq = self._state("arena_m", n_arena, dev), self._state("arena_v", n_arena, dev)
            check(lib.mae_engine_adamw_range(h, _ptr(m.flat_params), _ptr(m.flat_grads), _ptr(ea), _ptr(eq), _ptr(m._weights()), lr * scale,
                                             *hyper[1:5], step, _ptr(stats), p_lo, p_n, s))
        check(lib.mae_engine_adamw_buffer(h, _ptr(clf.head.flat), _ptr(head_g), _ptr(self._state("head_m", head_g.numel(), dev)),
                                          _ptr(self._state("head_v", head_g.numel(), dev)), head_g.numel(), *hyper[:5], step, _ptr(stats), s))
        if te:
            _n, pos_off, pos_n, _s, _f = m._offsets["encoder.vit.pos_embed"]
            skip = pos_row0 * m._dims["embed_dim"]  # the class-token row of a patch-only encoder stays as it is
            check(lib.mae_engine_adamw_buffer(h, _ptr(m.flat_params[pos_off + skip:pos_off + pos_n]), _ptr(pos_g[skip:]),
                                              _ptr(self._state("pos_m", pos_n, dev)[skip:]), _ptr(self._state("pos_v", pos_n, dev)[skip:]),
                                              pos_n - skip, lr * self.layer_scale(0), *hyper[1:5], step, _ptr(stats), s))
        if hi > lo:
            check(lib.mae_engine_refresh_transposed_range(h, _ptr(m.flat_params), _ptr(m._weights()), lo, hi - lo, s))
        m.mark_weights_fresh()
        return stats[:2]

    def _stash_grads(self, into_stash: bool, overwrite: bool = False) -> None:
        """The window's running sums of the three gradient buffers the optimizer reads: the arena range of the trainable set,
        ``head_grads`` and, when the embeddings train, ``pos_grads``.  ``into_stash``: stash (+)= live gradients; else live
        gradients += stash (the micro-batch that closes the window)."""
        tb, te = self._last_mode
        m = self.model.mae
        dev = m._require_cuda()
        head_g, pos_g = self._grad_buffers()
        lo, hi = self._arena_range(tb, te)
        pairs = [("arena", m.flat_grads[lo:hi]), ("head", head_g)] + ([("pos", pos_g)] if te else [])
        for key, live in pairs:
            if live.numel() == 0:
                continue
            st = self._stashes.get(key)
            if st is None or st.device != dev or st.numel() != live.numel():
                if not into_stash:
                    raise RuntimeError("the trainable set changed inside a window of micro-batches")
                st = self._stashes[key] = torch.zeros(live.numel(), dtype=torch.float32, device=dev)
            dst, src = (st, live) if into_stash else (live, st)
            check(lib.mae_engine_grad_accumulate(m.engine.handle, _ptr(dst), _ptr(src), 0, live.numel(), int(overwrite), _stream(dev)))

    def fused_training_step(self, images: torch.Tensor, labels: torch.Tensor, lr: Optional[float] = None,
                            accumulate: Optional[Tuple[int, int]] = None, window_rows: Optional[int] = None):
        """training_step + clip + AdamW, all native; returns device (loss, correct).  With mixup / CutMix configured the batch
        is mixed first (the draw is a function of (mix_seed, current_epoch, step)), and ``correct`` -- so the logged
        train_acc -- is counted against the batch's own labels, the first of each mixed pair.
        ``accumulate=(index, count)`` with ``window_rows`` (the rows of all the window's micro-batches): this batch is
        micro-batch ``index`` of a window that feeds ONE optimizer step.  Its loss gradient is weighted by rows / window_rows;
        every micro-batch but the last adds its gradients to a stash and returns its own (loss, correct), the last one adds the
        stash back, steps, logs train_loss / train_acc once for the window and returns the window's (mean loss, correct).  The
        augmentation, mixup / CutMix and drop-path draws stay per micro-batch.  None or a count of 1: the plain step."""
        window = self._window.enter(accumulate, window_rows)
        images = self._augment(images)
        rows = int(images.shape[0])
        weight = 1.0 if window is None else rows / float(window_rows)
        scale = self._draw_branch_scale(rows)
        if self.mixup_alpha > 0 or self.cutmix_alpha > 0:
            from .data import draw_mix_params, mix_batch
            params = draw_mix_params(rows, images.shape[-1], (self.mix_seed, self.current_epoch, self._mix_step),
                                     self.mixup_alpha, self.cutmix_alpha, self.mix_prob, self.mix_switch_prob)
            self._mix_step += 1
            m = self.model.mae
            images = m._check_images(images).to(m._require_cuda())
            images, labels, labels_b, lam = mix_batch(images, labels.to(images.device), params)
            loss, correct = self.loss_and_grads(images, labels, grad_scale=weight, labels_b=labels_b, lam=lam, branch_scale=scale)
        else:
            loss, correct = self.loss_and_grads(images, labels, grad_scale=weight, branch_scale=scale)
        if window is not None:
            index, count = window
            if index == 0:  # the window's rows-weighted loss and summed correct, on the device
                self._win_loss, self._win_correct = loss * weight, correct.clone()
            else:
                self._win_loss += loss * weight
                self._win_correct += correct
            if index < count - 1:
                self._stash_grads(into_stash=True, overwrite=index == 0)
                self._window.advance(index, count)
                return loss, correct
            self._stash_grads(into_stash=False)
            self._window.advance(index, count)
            loss, correct, rows = self._win_loss, self._win_correct, int(window_rows)
        self.optimizer_step(lr)
        self.log("train_loss", loss[0])
        self.log("train_acc", correct[0].float() / rows)
        return loss, correct

    # ---- checkpoints -------------------------------------------------------------------------------
    def checkpoint(self, epoch: int = 0, global_step: int = 0) -> Dict[str, Any]:
        """Lightning-shaped: state_dict keys model.encoder.<timm name> / model.head.classification.*.  ``hyper_parameters``
        gains ``with_cls: False`` for a patch-only encoder (with a class token the key set is the reference's, unchanged);
        ``checkpoint_with_cls`` reads it back."""
        return {"epoch": epoch, "global_step": global_step,
                "state_dict": {k: v.detach().cpu().clone() for k, v in self.state_dict().items()},
                "hyper_parameters": dict(self.hparams) if self.model.with_cls else dict(self.hparams, with_cls=False)}


def checkpoint_with_cls(ckpt: Dict[str, Any]) -> bool:
    """Whether a classifier checkpoint's encoder runs over [cls | patches] (True, also when the key is missing: every
    checkpoint written before the key existed) or over the patch tokens alone."""
    hp = ckpt.get("hyper_parameters") if isinstance(ckpt, dict) else None
    return bool((hp or {}).get("with_cls", True))


def encoder_mae(model_cfg: Dict[str, Any]) -> MaskedAutoencoder:
    """An engine MAE whose encoder is the classifier's; the decoder (unused here) is the smallest valid one unless the
    config names it."""
    g = dict(model_cfg.get("general", {}))
    e = dict(model_cfg.get("encoder", {}))
    d = model_cfg.get("decoder") or {}
    if "engine_precision" not in g and "engine" in model_cfg:
        g["engine_precision"] = model_cfg["engine"].get("precision", "bf16")
    if not d:
        d = dict(decoder_embed_dim=int(e.get("embed_dim", 384)), decoder_depth=1, decoder_num_heads=int(e.get("num_heads", 6)))
    return MaskedAutoencoder(g, e, d)


@torch.no_grad()
def build_baseline_encoder(model_cfg: Dict[str, Any], seed: Optional[int] = None) -> _ViT:
    """The reference's randomly initialised timm VisionTransformer (src/training/classifier.py:46-56), initialised as
    timm 1.0.21 ``VisionTransformer.init_weights('')`` does: Linear weights trunc_normal(std .02) with zero bias,
    LayerNorm 1 / 0, pos_embed trunc_normal(std .02) (trainable), cls_token normal(std 1e-6), and the patch Conv2d at
    PyTorch's default init (kaiming_uniform(a=sqrt 5) weight, uniform(+-1/sqrt(fan_in)) bias)."""
    mae = encoder_mae(model_cfg)
    g = torch.Generator().manual_seed(seed) if seed is not None else None
    vit = mae.encoder.vit
    for name, p in vit.named_parameters():
        if name == "pos_embed":
            p.copy_(_trunc_normal(p.shape, 0.02, g))
        elif name == "cls_token":
            p.copy_(torch.randn(p.shape, generator=g) * 1e-6)
        elif name.startswith("patch_embed.proj."):
            fan_in = int(torch.tensor(vit.patch_embed.proj.weight.shape[1:]).prod())
            bound = 1.0 / math.sqrt(fan_in)  # kaiming_uniform(a=sqrt(5)) on the weight gives the same bound
            p.copy_((torch.rand(p.shape, generator=g) * 2 - 1) * bound)
        elif name.startswith("norm") or ".norm" in name:
            p.fill_(1.0 if name.endswith("weight") else 0.0)
        elif name.endswith("weight"):
            p.copy_(_trunc_normal(p.shape, 0.02, g))
        else:
            p.zero_()
    vit.pos_embed.requires_grad = True
    return vit


def _trunc_normal(shape, std: float, g: Optional[torch.Generator]) -> torch.Tensor:
    """torch.nn.init.trunc_normal_(std=std, a=-2, b=2) (timm's call: the cut is at +-2 absolute, i.e. +-100 sigma here)."""
    t = torch.empty(shape)
    torch.nn.init.trunc_normal_(t, std=std, a=-2.0, b=2.0, generator=g)
    return t


def load_encoder_weights(mae: MaskedAutoencoder, state: Dict[str, torch.Tensor]) -> Tuple[List[str], List[str]]:
    """scripts/training/train_mae.py:111-135: strip the first of ``model.encoder.`` / ``encoder.`` / ``module.encoder.``
    that matches and load into ``mae.encoder`` with strict=False; returns (missing, unexpected)."""
    for pfx in ("model.encoder.", "encoder.", "module.encoder."):
        sub = {k[len(pfx):]: v for k, v in state.items() if k.startswith(pfx)}
        if sub:
            break
    else:
        sub = dict(state)
    res = mae.encoder.load_state_dict(sub, strict=False)
    return list(res.missing_keys), list(res.unexpected_keys)
