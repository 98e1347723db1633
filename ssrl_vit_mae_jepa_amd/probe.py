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


def parse_block(block: Optional[Dict[str, Any]], defaults: Dict[str, Any], name: str, int_keys, float_keys) -> Dict[str, Any]:
    """The YAML block ``name:`` completed with ``defaults``: it must be a mapping, an unknown key is refused by name, a ``None`` value
    keeps its default, and ``int_keys`` / ``float_keys`` are cast.  The range checks are the caller's."""
    block = block or {}
    if not isinstance(block, dict):
        raise ValueError(f"{name} must be a mapping, got {block!r}")
    unknown = set(block) - set(defaults)
    if unknown:
        raise ValueError(f"{name}: unknown keys {sorted(unknown)}")
    out = dict(defaults)
    out.update({k: v for k, v in block.items() if v is not None})
    for k in int_keys:
        out[k] = int(out[k])
    for k in float_keys:
        out[k] = float(out[k])
    return out


def parse_probe(block: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The YAML block ``probe:`` checked and completed with ``PROBE_DEFAULTS``; an unknown key is refused by name."""
    out = parse_block(block, PROBE_DEFAULTS, "probe", ("total_epochs", "warmup_epochs", "batch_size"),
                      ("base_learning_rate", "weight_decay", "momentum", "trust_coefficient", "bn_eps", "bn_momentum", "head_init_std"))
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


class _Probe:
    """What ``LinearProbe``, ``ProbeSweep`` and ``attentive.AttentiveProbe`` share: the scratch pool, the check of a batch and the
    BatchNorm and classifier-head calls.  A subclass has ``device``, ``dim``, ``num_classes``, ``cfg`` (bn_eps, bn_momentum) and a
    ``_scratch`` dict that ``to()`` clears."""

    # whose kernels, the class the device message names, the input's word, its leading axes, what a label belongs to
    _INPUT = ("the probe's", "LinearProbe", "features", ("B",), "feature rows")

    def _bytes(self, key: str, need: int) -> torch.Tensor:
        """The pool's buffer ``key`` with at least ``need`` bytes: it only grows, so a smaller call reuses the larger buffer."""
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < need or buf.device != self.device:
            buf = self._scratch[key] = torch.empty(max(int(need), 16), dtype=torch.uint8, device=self.device)
        return buf

    def _f32(self, key: str, *shape: int) -> torch.Tensor:
        n = 1
        for s in shape:
            n *= int(s)
        return self._bytes(key, 4 * n)[:4 * n].view(torch.float32).view(*shape)

    def _check(self, x: torch.Tensor, labels: Optional[torch.Tensor]):
        """(x fp32 contiguous, labels int64 flat or None) of a batch on the probe's device, one label per leading row."""
        whose, cls, word, lead, rows = self._INPUT
        if not x.is_cuda:
            raise RuntimeError(f"{whose} kernels run on the MI355X only (move the {word} to cuda)")
        if self.device != x.device:
            raise RuntimeError(f"{cls}: move the probe to the {word}' device with .to(device)")
        if x.dim() != len(lead) + 1 or x.shape[-1] != self.dim:
            raise ValueError(f"{word} must be ({', '.join(lead)}, {self.dim}), got {tuple(x.shape)}")
        x = x.to(dtype=torch.float32).contiguous()
        if labels is not None:
            labels = labels.to(device=x.device, dtype=torch.int64).contiguous().view(-1)
            if labels.numel() != x.shape[0]:
                raise ValueError(f"{labels.numel()} labels for {x.shape[0]} {rows}")
        return x, labels

    def _batchnorm(self, x: torch.Tensor, running_mean, running_var, training: bool, mean, rstd, y=None) -> None:
        """BatchNorm over all rows of ``x`` (every axis but the last) on the given running buffers: ``mean`` and ``rstd`` always, the
        normalised rows too where ``y`` is given (``mae_batchnorm_fwd``, else ``mae_batchnorm_stats``)."""
        D = x.shape[-1]
        rows = x.numel() // D
        need = lib.mae_batchnorm_scratch_bytes(rows, D)
        if need < 0:
            raise ValueError(f"BatchNorm shape ({rows}, {D}) outside the kernel's limits")
        scratch = self._bytes("bn", need)
        head = (_ptr(x), rows, D, self.cfg["bn_eps"], int(training), self.cfg["bn_momentum"], _ptr(running_mean), _ptr(running_var))
        tail = (_ptr(mean), _ptr(rstd), _ptr(scratch), scratch.numel(), _stream(x.device))
        check(lib.mae_batchnorm_stats(*head, *tail) if y is None else lib.mae_batchnorm_fwd(*head, _ptr(y), *tail))

    def _classifier_head(self, rows: torch.Tensor, flat: torch.Tensor, labels: Optional[torch.Tensor], grads=None, d_feats=None):
        """``mae_classifier_head`` on (B, D) fp32 rows (seq_len 1, the class-row pool) with the flat W-then-b head ``flat``: (logits,
        loss or None, correct or None); ``grads`` takes dW then db, ``d_feats`` the gradient of the rows."""
        B, D = rows.shape
        dev, C = rows.device, self.num_classes
        logits = torch.empty(B, C, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev) if labels is not None else None
        correct = torch.empty(1, dtype=torch.int32, device=dev) if labels is not None else None
        need = lib.mae_classifier_head_scratch_bytes(B, C, D)
        if need < 0:
            raise ValueError(f"head shape (batch {B}, classes {C}, dim {D}) outside the kernel's limits")
        scratch = self._bytes("head", need + 256)
        off = (-scratch.data_ptr()) % 256
        scratch = scratch[off:off + need]
        check(lib.mae_classifier_head(_ptr(rows), _lib.MAE_F32, B, 1, D, _lib.POOL_CLS, _ptr(flat), C, _ptr(labels), 1.0, _ptr(logits),
                                      _ptr(loss), _ptr(correct), _ptr(grads), _ptr(d_feats), _ptr(scratch), need, _stream(dev)))
        return logits, loss, correct


class _FeatureProbe(_Probe):
    """A probe on (B, dim) feature rows behind one BatchNorm, ``self.bn``."""

    def _normalise(self, feats: torch.Tensor, training: bool) -> torch.Tensor:
        D, dev = feats.shape[1], feats.device
        y = torch.empty_like(feats)   # the cached features are read again next epoch: never in place here
        mean, rstd = torch.empty(D, dtype=torch.float32, device=dev), torch.empty(D, dtype=torch.float32, device=dev)
        self._batchnorm(feats, self.bn.running_mean, self.bn.running_var, training, mean, rstd, y)
        self.last.update(y=y, mean=mean, rstd=rstd)
        return y


class LinearProbe(_FeatureProbe):
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

    @property
    def bn(self) -> _BatchNormStats:
        return self.head.bn

    # ---- the three operations ------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, feats: torch.Tensor, labels: torch.Tensor, lr: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step on a batch of at least two rows: (loss (1,) fp32, correct (1,) int32), device tensors, no synchronisation."""
        feats, labels = self._check(feats, labels)
        if feats.shape[0] < 2:
            raise ValueError("a probe step needs at least 2 rows (BatchNorm in training mode)")
        y = self._normalise(feats, True)
        self.bn.num_batches_tracked += 1
        flat = self.head.flat
        logits, loss, correct = self._classifier_head(y, flat, labels, self.grads)
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
        feats, labels = self._check(feats, labels)
        return self._classifier_head(self._normalise(feats, False), self.head.flat, labels)

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


# ----------------------------------------------------------------------------------------------------------------------
# the sweep: a grid of heads on the same features in one pass
# ----------------------------------------------------------------------------------------------------------------------
SWEEP_MAX_HEADS = 64
SWEEP_AXES = ("base_learning_rate", "weight_decay")


def _sweep_axis(name: str, value) -> list:
    """One axis of the grid: a comma-separated string (a flag), a list (the YAML) or a single number."""
    if isinstance(value, str):
        items = [v.strip() for v in value.split(",")]
        if not value.strip() or any(not v for v in items):
            raise ValueError(f"probe sweep: {name} must be a comma-separated list of numbers, got {value!r}")
    elif isinstance(value, (list, tuple)):
        items = list(value)
    else:
        items = [value]
    if not items:
        raise ValueError(f"probe sweep: {name} is empty")
    out = []
    for v in items:
        try:
            if isinstance(v, bool):
                raise TypeError
            out.append(float(v))
        except (TypeError, ValueError):
            raise ValueError(f"probe sweep: {name} holds {v!r}, which is no number") from None
    for v in out:
        if not np.isfinite(v) or (v <= 0 if name == "base_learning_rate" else v < 0):
            raise ValueError(f"probe sweep: {name} = {v} ({'must be > 0' if name == 'base_learning_rate' else 'must be >= 0'})")
    if len(set(out)) != len(out):
        raise ValueError(f"probe sweep: {name} repeats a value: {out}")
    return out


def parse_sweep(block: Optional[Dict[str, Any]], cfg: Dict[str, Any], sweep_lr=None, sweep_wd=None) -> Optional[list]:
    """The grid of a sweep, or None when none is asked for.  ``block`` is the top-level YAML block ``probe_sweep:`` (lists under
    ``base_learning_rate`` / ``weight_decay``), ``sweep_lr`` / ``sweep_wd`` the flags' comma-separated strings: a flag overrides its
    key, a missing axis takes the single value of ``cfg`` (a ``parse_probe`` result).  The grid is the product, learning rate
    outermost: a list of {base_learning_rate, weight_decay}.  More than SWEEP_MAX_HEADS heads are refused by name."""
    if block is None and sweep_lr is None and sweep_wd is None:
        return None
    block = {} if block is None else block
    if not isinstance(block, dict):
        raise ValueError(f"probe_sweep must be a mapping, got {block!r}")
    unknown = set(block) - set(SWEEP_AXES)
    if unknown:
        raise ValueError(f"probe_sweep: unknown keys {sorted(unknown)}")
    given = dict(base_learning_rate=sweep_lr, weight_decay=sweep_wd)
    axes = {}
    for name in SWEEP_AXES:
        value = given[name] if given[name] is not None else block.get(name)
        axes[name] = _sweep_axis(name, cfg[name] if value is None else value)
    heads = len(axes["base_learning_rate"]) * len(axes["weight_decay"])
    if heads > SWEEP_MAX_HEADS:
        raise ValueError(f"probe sweep: {len(axes['base_learning_rate'])} learning rates x {len(axes['weight_decay'])} weight decays = {heads} heads; "
                         f"one sweep takes at most {SWEEP_MAX_HEADS}")
    return [dict(base_learning_rate=lr, weight_decay=wd) for lr in axes["base_learning_rate"] for wd in axes["weight_decay"]]


def select(val_acc, val_loss) -> int:
    """The winner of a sweep: the highest validation accuracy; ties go to the lower validation loss, then to the lower index.
    A loss that is not finite loses every tie."""
    if len(val_acc) != len(val_loss) or len(val_acc) == 0:
        raise ValueError(f"select: {len(val_acc)} accuracies and {len(val_loss)} losses")
    key = lambda g: (-float(val_acc[g]), float(val_loss[g]) if np.isfinite(float(val_loss[g])) else float("inf"), g)
    return min(range(len(val_acc)), key=key)


class ProbeSweep(_FeatureProbe):
    """G linear probes that differ in learning rate and weight decay alone, trained on the same features in one pass: one shared
    BatchNorm (it has no per-head state), a stacked (G, HF) parameter, momentum and gradient buffer, ``mae_probe_sweep_head`` for
    every head's logits, loss and gradients and ``mae_lars_step_groups`` for every head's update.  ``grid``: a list of
    {base_learning_rate, weight_decay} (``parse_sweep``); everything else comes from ``cfg``, a ``parse_probe`` result shared by all
    heads.  Every head starts from the weights ``ProbeHead(seed)`` has."""

    def __init__(self, dim: int, num_classes: int, grid, cfg: Optional[Dict[str, Any]] = None, seed: Optional[int] = 73, device=None):
        self.cfg = parse_probe(cfg)
        self.grid = [dict(base_learning_rate=float(g["base_learning_rate"]), weight_decay=float(g["weight_decay"])) for g in grid]
        if not 1 <= len(self.grid) <= SWEEP_MAX_HEADS:
            raise ValueError(f"a probe sweep has 1 to {SWEEP_MAX_HEADS} heads, got {len(self.grid)}")
        if any(not (g["base_learning_rate"] > 0 and g["weight_decay"] >= 0) for g in self.grid):
            raise ValueError("probe sweep: base_learning_rate > 0 and weight_decay >= 0 in every head")
        proto = ProbeHead(dim, num_classes, self.cfg["head_init_std"], seed)
        self.dim, self.num_classes, self.seed = proto.dim, proto.num_classes, seed
        self.bn = _BatchNormStats(self.dim)
        self.head_floats = proto.flat.numel()
        self.flat = proto.flat.detach().clone().unsqueeze(0).repeat(len(self.grid), 1).contiguous()   # (G, HF)
        self.mu = torch.zeros_like(self.flat)
        self.grads = torch.zeros_like(self.flat)
        self.steps = 0
        self.epoch = 0
        self._scratch: Dict[str, torch.Tensor] = {}
        self.last: Dict[str, torch.Tensor] = {}   # y, mean, rstd, logits (G, B, C) of the latest step
        if device is not None:
            self.to(device)

    def __len__(self) -> int:
        return len(self.grid)

    def to(self, device) -> "ProbeSweep":
        self.bn.to(device)
        self.flat, self.mu, self.grads = self.flat.to(device), self.mu.to(device), self.grads.to(device)
        self._scratch.clear()
        return self

    @property
    def device(self) -> torch.device:
        return self.flat.device

    def _heads(self, rows: torch.Tensor, labels: Optional[torch.Tensor], grads: Optional[torch.Tensor], want_logits: bool = True):
        B, D = rows.shape
        dev, C, G = rows.device, self.num_classes, len(self.grid)
        logits = torch.empty(G, B, C, dtype=torch.float32, device=dev) if want_logits or labels is None else None
        loss = torch.empty(G, dtype=torch.float32, device=dev) if labels is not None else None
        correct = torch.empty(G, dtype=torch.int32, device=dev) if labels is not None else None
        need = lib.mae_probe_sweep_scratch_bytes(B, D, C, G)
        if need < 0:
            raise ValueError(f"sweep shape (rows {B}, dim {D}, classes {C}, heads {G}) outside the kernel's limits")
        scratch = self._bytes("head", need)
        if labels is not None and labels.data_ptr() % 16:   # a slice of a label vector at an odd row: the kernels take 16-byte aligned buffers
            labels = labels.clone()
        check(lib.mae_probe_sweep_head(_ptr(rows), B, D, _ptr(self.flat), G, C, _ptr(labels), _ptr(logits), _ptr(loss), _ptr(correct), _ptr(grads),
                                       _ptr(scratch), scratch.numel(), _stream(dev)))
        return logits, loss, correct

    def head_lrs(self, lr_factor: float = 1.0) -> np.ndarray:
        """fp32 learning rate per head: probe_lr(head) * lr_factor, formed in double and rounded once."""
        bs = int(self.cfg["batch_size"])
        return np.array([float(g["base_learning_rate"]) * bs / 256.0 * float(lr_factor) for g in self.grid], dtype=np.float64).astype(np.float32)

    # ---- the operations ------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, feats: torch.Tensor, labels: torch.Tensor, lr_factor: float = 1.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step of every head on a batch of at least two rows: (loss (G,) fp32, correct (G,) int32), device tensors, no
        synchronisation.  One BatchNorm, one sweep head, two grouped LARS calls (W with the trust ratio, then the bias slice)."""
        feats, labels = self._check(feats, labels)
        if feats.shape[0] < 2:
            raise ValueError("a probe step needs at least 2 rows (BatchNorm in training mode)")
        y = self._normalise(feats, True)
        self.bn.num_batches_tracked += 1
        logits, loss, correct = self._heads(y, labels, self.grads)
        self.last["logits"] = logits
        c, G, HF = self.cfg, len(self.grid), self.head_floats
        nw = self.num_classes * self.dim
        dev = feats.device
        lrs = self.head_lrs(lr_factor)
        wds = np.array([g["weight_decay"] for g in self.grid], dtype=np.float32)
        ls = self._bytes("lars", G * LARS_SCRATCH_FLOATS * 4).view(torch.float32)
        flat, grads, mu = self.flat.view(-1), self.grads.view(-1), self.mu.view(-1)
        for lo, hi, adapt in ((0, nw, 1), (nw, HF, 0)):   # W with the trust ratio, then the bias slice (padding included)
            check(lib.mae_lars_step_groups(_ptr(flat[lo:]), _ptr(grads[lo:]), _ptr(mu[lo:]), G, HF, hi - lo, adapt, lrs.ctypes.data, wds.ctypes.data,
                                           c["momentum"], c["trust_coefficient"], None, _ptr(ls), ls.numel(), _stream(dev)))
        self.steps += 1
        return loss, correct

    @torch.no_grad()
    def evaluate(self, feats: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """(logits (G, B, C), loss (G,) or None, correct (G,) or None) with the running statistics; changes no state."""
        feats, labels = self._check(feats, labels)
        return self._heads(self._normalise(feats, False), labels, None)

    def export(self, g: int) -> LinearProbe:
        """Head g as a ``LinearProbe`` of its own: its weights, momentum, hyper-parameters and the shared BatchNorm buffers (copies), so
        ``folded_head`` / ``classifier_checkpoint`` write it as they write any probe."""
        g = int(g)
        if not 0 <= g < len(self.grid):
            raise IndexError(f"head {g} of a sweep of {len(self.grid)}")
        probe = LinearProbe(self.dim, self.num_classes, dict(self.cfg, **self.grid[g]), seed=self.seed, device=self.device)
        with torch.no_grad():
            probe.head.flat.copy_(self.flat[g])
            probe.mu.copy_(self.mu[g])
            for k in ("running_mean", "running_var", "num_batches_tracked"):
                getattr(probe.head.bn, k).copy_(getattr(self.bn, k))
        probe.steps, probe.epoch = self.steps, self.epoch
        return probe

    # ---- resume --------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        out = {"bn." + k: v.detach().cpu().clone() for k, v in self.bn.state_dict().items()}
        out.update(flat=self.flat.detach().cpu().clone(), mu=self.mu.detach().cpu().clone(), steps=int(self.steps), epoch=int(self.epoch),
                   cfg=dict(self.cfg), grid=[dict(g) for g in self.grid], dim=self.dim, num_classes=self.num_classes)
        return out

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, Any]) -> None:
        if "grid" not in state or [dict(g) for g in state["grid"]] != self.grid:
            raise ValueError(f"the state's grid {state.get('grid')} differs from this sweep's {self.grid}")
        if tuple(state["flat"].shape) != tuple(self.flat.shape):
            raise ValueError(f"the state holds heads of shape {tuple(state['flat'].shape)}, the sweep {tuple(self.flat.shape)}")
        self.bn.load_state_dict({k[len("bn."):]: v for k, v in state.items() if k.startswith("bn.")}, strict=True)
        self.flat.copy_(state["flat"].to(self.device))
        self.mu.copy_(state["mu"].to(self.device))
        self.steps, self.epoch = int(state["steps"]), int(state["epoch"])
