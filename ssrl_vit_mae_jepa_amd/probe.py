"""Linear probing on cached features: the protocol of the MAE paper (A.1, Table 10) and of I-JEPA.

A frozen encoder gives the same features every epoch, so they are extracted once (``representation.extract_split_features``)
and the probe trains on them: ``BatchNorm1d(D, affine=False, eps=1e-6)`` on the pooled feature, a linear layer, LARS without
weight decay (momentum 0.9, trust coefficient 0.001, no gradient clipping), no augmentation beyond RandomResizedCrop + flip.

``LinearProbe.step`` is three native calls: ``mae_batchnorm_fwd`` (training mode), ``mae_classifier_head`` on the normalised rows
(fp32, seq_len 1, the class-row pool: logits, cross-entropy, dW and db) and ``mae_lars_step`` on the weight (with the trust
ratio) and on the bias (without).  Nothing synchronises with the host.  ``folded_head`` folds the running statistics into the
linear layer, so the result is an ordinary classifier checkpoint that ``train_mae.build_module(classifier_ckpt=...)`` and
``scripts/evaluation/evaluate_classifier.py`` read unchanged.

The probe works on the feature pools of ``MaskedAutoencoder.extract_features``; ``CLASSIFIER_POOL`` maps them to the classifier's
names when a checkpoint is written.
"""
from __future__ import annotations

import copy
from typing import Any, Dict, Optional, Tuple

import numpy as np
import torch
from torch import nn

from . import _lib
from ._lib import check, lib
from .classifier import MAX_CLASSES, NO_CLS_POOL, ClassificationHead, _trunc_normal
from .mae import _ptr, _stream, _ViT

# feature pool (extract_features) -> classifier pool (ViTClassifier)
CLASSIFIER_POOL = {"cls": "cls", "mean": "mean_patches", "mean_all": "mean"}

PROBE_DEFAULTS: Dict[str, Any] = {
    "total_epochs": 90, "warmup_epochs": 10, "batch_size": 2000, "base_learning_rate": 0.1, "weight_decay": 0.0, "momentum": 0.9,
    "trust_coefficient": 0.001, "bn_eps": 1e-6, "bn_momentum": 0.1, "head_init_std": 0.01, "augment": "none"}
AUGMENTS = ("none", "crop")
LARS_SCRATCH_FLOATS = 4096


def parse_probe(block: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The YAML block ``probe:`` checked and completed with ``PROBE_DEFAULTS``; an unknown key is refused by name."""
    block = block or {}
    if not isinstance(block, dict):
        raise ValueError(f"probe must be a mapping, got {block!r}")
    unknown = set(block) - set(PROBE_DEFAULTS)
    if unknown:
        raise ValueError(f"probe: unknown keys {sorted(unknown)}")
    out = dict(PROBE_DEFAULTS)
    for k, v in block.items():
        if v is not None:
            out[k] = v
    for k in ("total_epochs", "warmup_epochs", "batch_size"):
        out[k] = int(out[k])
    for k in ("base_learning_rate", "weight_decay", "momentum", "trust_coefficient", "bn_eps", "bn_momentum", "head_init_std"):
        out[k] = float(out[k])
    if out["augment"] not in AUGMENTS:
        raise ValueError(f"probe.augment must be one of {list(AUGMENTS)}, got {out['augment']!r}")
    if out["total_epochs"] < 1 or out["warmup_epochs"] < 0 or out["batch_size"] < 2:
        raise ValueError("probe: total_epochs >= 1, warmup_epochs >= 0 and batch_size >= 2 (BatchNorm needs two rows)")
    if not (out["base_learning_rate"] > 0 and out["weight_decay"] >= 0 and 0 <= out["momentum"] < 1 and out["trust_coefficient"] > 0):
        raise ValueError("probe: base_learning_rate > 0, weight_decay >= 0, momentum in [0, 1), trust_coefficient > 0")
    if not (out["bn_eps"] >= 0 and 0 <= out["bn_momentum"] <= 1 and out["head_init_std"] > 0):
        raise ValueError("probe: bn_eps >= 0, bn_momentum in [0, 1], head_init_std > 0")
    return out


def probe_lr(cfg: Dict[str, Any]) -> float:
    """The recipe's peak learning rate: base_learning_rate * batch_size / 256."""
    return float(cfg["base_learning_rate"]) * int(cfg["batch_size"]) / 256.0


def classifier_pool(feature_pool: str, with_cls: bool = True) -> str:
    """The classifier pool that reads what the feature pool ``feature_pool`` produced; a patch-only encoder refuses ``cls``."""
    if feature_pool not in CLASSIFIER_POOL:
        raise ValueError(f"pool must be one of {sorted(CLASSIFIER_POOL)}, got {feature_pool!r}")
    if feature_pool == "cls" and not with_cls:
        raise ValueError(NO_CLS_POOL)
    return CLASSIFIER_POOL[feature_pool]


def fold(weight, bias, running_mean, running_var, eps: float) -> Tuple[np.ndarray, np.ndarray]:
    """BatchNorm's evaluation form folded into the linear layer, float64: W'[c][d] = W[c][d] / sqrt(var[d] + eps),
    b'[c] = b[c] - sum_d W'[c][d] mean[d]; eps enters as the fp32 value the kernel receives."""
    w, b = np.asarray(weight, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    m, v = np.asarray(running_mean, dtype=np.float64), np.asarray(running_var, dtype=np.float64)
    wf = w / np.sqrt(v + float(np.float32(eps)))[None, :]
    return wf, b - wf @ m


class _BatchNormStats(nn.Module):
    def __init__(self, dim: int) -> None:
        super().__init__()
        self.register_buffer("running_mean", torch.zeros(dim, dtype=torch.float32))
        self.register_buffer("running_var", torch.ones(dim, dtype=torch.float32))
        self.register_buffer("num_batches_tracked", torch.zeros((), dtype=torch.int64))


class ProbeHead(nn.Module):
    """BatchNorm1d(dim, affine=False) statistics (``bn.running_mean`` / ``bn.running_var`` / ``bn.num_batches_tracked``, initialised as
    torch's) in front of a ``ClassificationHead`` (``classification``, the flat W-then-b buffer the C ABI reads).  The weight starts
    as trunc_normal(std = head_init_std), the bias at zero: the recipe's init."""

    def __init__(self, dim: int, num_classes: int, head_init_std: float = 0.01, seed: Optional[int] = 73) -> None:
        super().__init__()
        if dim % 4 != 0 or not 4 <= dim <= 1024:
            raise ValueError(f"the probe needs a feature width that is a multiple of 4 in [4, 1024], got {dim}")
        if not 2 <= int(num_classes) <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [2, {MAX_CLASSES}], got {num_classes}")
        self.dim, self.num_classes = int(dim), int(num_classes)
        self.bn = _BatchNormStats(self.dim)
        self.classification = ClassificationHead(self.dim, self.num_classes)
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        with torch.no_grad():
            self.classification.classification.weight.copy_(_trunc_normal((self.num_classes, self.dim), float(head_init_std), g))
            self.classification.classification.bias.zero_()

    @property
    def flat(self) -> torch.Tensor:
        return self.classification.flat


def _encoder_state(encoder) -> Tuple[Dict[str, torch.Tensor], bool]:
    """(timm-named tensors, with_cls) of a ``_ViT`` node or a ``representation.EvalEncoder``."""
    if isinstance(encoder, _ViT):
        return dict(encoder.state_dict()), bool(encoder.with_cls)
    vit = getattr(encoder, "vit", None)
    if vit is not None:
        return dict(vit.state_dict()), bool(encoder.with_cls)
    model = getattr(encoder, "ijepa", None)
    if model is None:
        raise TypeError("classifier_checkpoint needs the engine's encoder node or an EvalEncoder")
    src = model.target_state_dict() if encoder.encoder == "target" else model.net.state_dict()
    pfx = "encoder.vit."
    return {k[len(pfx):]: v for k, v in src.items() if k.startswith(pfx)}, False


class LinearProbe:
    """The probe's state (a ``ProbeHead``, the LARS momentum buffer, the gradient and scratch buffers) and its three operations.
    ``cfg``: a ``parse_probe`` result (or a subset of its keys); features are (B, dim) fp32 rows on the device."""

    def __init__(self, dim: int, num_classes: int, cfg: Optional[Dict[str, Any]] = None, seed: Optional[int] = 73, device=None):
        self.cfg = parse_probe(cfg)
        self.head = ProbeHead(dim, num_classes, self.cfg["head_init_std"], seed)
        self.dim, self.num_classes = self.head.dim, self.head.num_classes
        n = self.head.flat.numel()
        self.mu = torch.zeros(n, dtype=torch.float32)
        self.grads = torch.zeros(n, dtype=torch.float32)   # dW then db; the padding stays zero
        self.steps = 0
        self.epoch = 0
        self._scratch: Dict[str, torch.Tensor] = {}
        self.last: Dict[str, torch.Tensor] = {}             # y, mean, rstd, logits of the latest step (the tests read them)
        if device is not None:
            self.to(device)

    def to(self, device) -> "LinearProbe":
        self.head.to(device)
        self.mu, self.grads = self.mu.to(device), self.grads.to(device)
        self._scratch.clear()
        return self

    @property
    def device(self) -> torch.device:
        return self.head.flat.device

    # ---- buffers -----------------------------------------------------------------------------------
    def _bytes(self, key: str, need: int) -> torch.Tensor:
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < need or buf.device != self.device:
            buf = self._scratch[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=self.device)
        return buf

    def _check_feats(self, feats: torch.Tensor, labels: Optional[torch.Tensor]):
        if not feats.is_cuda:
            raise RuntimeError("the probe's kernels run on the MI355X only (move the features to cuda)")
        if self.device != feats.device:
            raise RuntimeError("LinearProbe: move the probe to the features' device with .to(device)")
        if feats.dim() != 2 or feats.shape[1] != self.dim:
            raise ValueError(f"features must be (B, {self.dim}), got {tuple(feats.shape)}")
        feats = feats.to(dtype=torch.float32).contiguous()
        if labels is not None:
            labels = labels.to(device=feats.device, dtype=torch.int64).contiguous().view(-1)
            if labels.numel() != feats.shape[0]:
                raise ValueError(f"{labels.numel()} labels for {feats.shape[0]} feature rows")
        return feats, labels

    def _batchnorm(self, feats: torch.Tensor, training: bool) -> torch.Tensor:
        B, D = feats.shape
        bn, dev = self.head.bn, feats.device
        y = torch.empty_like(feats)   # the cached features are read again next epoch: never in place here
        need = lib.mae_batchnorm_scratch_bytes(B, D)
        if need < 0:
            raise ValueError(f"BatchNorm shape ({B}, {D}) outside the kernel's limits")
        scratch = self._bytes("bn", need)
        mean, rstd = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        check(lib.mae_batchnorm_fwd(_ptr(feats), B, D, self.cfg["bn_eps"], int(training), self.cfg["bn_momentum"], _ptr(bn.running_mean),
                                    _ptr(bn.running_var), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(scratch), scratch.numel(), _stream(dev)))
        self.last.update(y=y, mean=mean, rstd=rstd)
        return y

    def _head(self, rows: torch.Tensor, flat: torch.Tensor, labels: Optional[torch.Tensor], grads: Optional[torch.Tensor]):
        B, D = rows.shape
        dev, C = rows.device, self.num_classes
        logits = torch.empty(B, C, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev) if labels is not None else None
        correct = torch.empty(1, dtype=torch.int32, device=dev) if labels is not None else None
        need = lib.mae_classifier_head_scratch_bytes(B, C, D)
        scratch = self._bytes("head", need + 256)
        off = (-scratch.data_ptr()) % 256
        scratch = scratch[off:off + need]
        check(lib.mae_classifier_head(_ptr(rows), _lib.MAE_F32, B, 1, D, _lib.POOL_CLS, _ptr(flat), C, _ptr(labels), 1.0, _ptr(logits),
                                      _ptr(loss), _ptr(correct), _ptr(grads), None, _ptr(scratch), need, _stream(dev)))
        return logits, loss, correct

    # ---- the three operations ------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, feats: torch.Tensor, labels: torch.Tensor, lr: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step on a batch of at least two rows: (loss (1,) fp32, correct (1,) int32), device tensors, no synchronisation."""
        feats, labels = self._check_feats(feats, labels)
        if feats.shape[0] < 2:
            raise ValueError("a probe step needs at least 2 rows (BatchNorm in training mode)")
        y = self._batchnorm(feats, True)
        self.head.bn.num_batches_tracked += 1
        flat = self.head.flat
        logits, loss, correct = self._head(y, flat, labels, self.grads)
        self.last["logits"] = logits
        c = self.cfg
        nw = self.num_classes * self.dim
        dev = feats.device
        ls = self._bytes("lars", LARS_SCRATCH_FLOATS * 4).view(torch.float32)
        for lo, hi, adapt in ((0, nw, 1), (nw, flat.numel(), 0)):   # W with the trust ratio, then the bias slice (padding included)
            check(lib.mae_lars_step(_ptr(flat[lo:hi]), _ptr(self.grads[lo:hi]), _ptr(self.mu[lo:hi]), hi - lo, adapt, float(lr), c["momentum"],
                                    c["weight_decay"], c["trust_coefficient"], None, _ptr(ls), _stream(dev)))
        self.steps += 1
        return loss, correct

    @torch.no_grad()
    def evaluate(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """(logits, loss or None, correct or None) with the running statistics; changes no state."""
        feats, labels = self._check_feats(feats, labels)
        y = self._batchnorm(feats, False)
        return self._head(y, self.head.flat, labels, None)

    def folded_head(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(W' (C, D), b' (C,)) fp32 on the host: BatchNorm's evaluation form folded into the linear layer, computed in float64 and
        rounded once."""
        lin, bn = self.head.classification.classification, self.head.bn
        wf, bf = fold(lin.weight.detach().cpu().numpy(), lin.bias.detach().cpu().numpy(), bn.running_mean.cpu().numpy(),
                      bn.running_var.cpu().numpy(), self.cfg["bn_eps"])
        return torch.from_numpy(wf.astype(np.float32)), torch.from_numpy(bf.astype(np.float32))

    def classifier_checkpoint(self, encoder, model_cfg: Dict[str, Any], pool: str, epoch: int = 0) -> Dict[str, Any]:
        """A Lightning-shaped classifier checkpoint of ``encoder`` (the engine's ViT node or an ``EvalEncoder``) with the folded head:
        keys model.encoder.<timm name> and model.head.classification.*; ``hyper_parameters`` carries model_cfg with head.pool set to
        the classifier's name of the feature pool ``pool``, num_classes, and with_cls (always written)."""
        state, with_cls = _encoder_state(encoder)
        cpool = classifier_pool(pool, with_cls)
        w, b = self.folded_head()
        sd = {"model.encoder." + k: v.detach().cpu().clone() for k, v in state.items()}
        sd["model.head.classification.weight"], sd["model.head.classification.bias"] = w, b
        cfg = copy.deepcopy(dict(model_cfg))
        cfg["head"] = dict(cfg.get("head") or {}, pool=cpool)
        return {"epoch": int(epoch), "global_step": int(self.steps), "state_dict": sd,
                "hyper_parameters": {"model_cfg": cfg, "training_cfg": {}, "num_classes": self.num_classes, "with_cls": bool(with_cls)}}

    # ---- resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        out = {"head." + k: v.detach().cpu().clone() for k, v in self.head.state_dict().items()}
        out.update(mu=self.mu.detach().cpu().clone(), steps=int(self.steps), epoch=int(self.epoch), cfg=dict(self.cfg))
        return out

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, Any]) -> None:
        head = {k[len("head."):]: v for k, v in state.items() if k.startswith("head.")}
        self.head.load_state_dict(head, strict=True)
        if state["mu"].numel() != self.mu.numel():
            raise ValueError(f"mu has {state['mu'].numel()} elements, the probe {self.mu.numel()}")
        self.mu.copy_(state["mu"].to(self.mu.device))
        self.steps, self.epoch = int(state["steps"]), int(state["epoch"])
