"""Representation quality of frozen encoders: pooled features, the weighted k-NN probe and the checkpoint loader behind
``scripts/evaluation/knn_eval.py`` and ``scripts/evaluation/visualize_representation.py``.

Features come from the engine (``mae_engine_extract_features``); the k-NN search and vote are the HIP kernels of
k_representation.hip (``mae_knn_topk`` / ``mae_knn_vote``).  Only ``apply_normalization`` and the checkpoint
bookkeeping run on the host.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, Iterable, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import check, lib
from .classifier import build_baseline_encoder, checkpoint_with_cls, encoder_mae
from .mae import _ViT, _stream

_ptr = _lib.ptr

KNN_MAX_K = 256
KNN_MAX_DIM = 4096  # columns mae_knn_topk takes
DEFAULT_KS = (10, 20, 100, 200)


# ---------------------------------------------------------------------------------------------------------------------
# k-NN
# ---------------------------------------------------------------------------------------------------------------------
def _f32_rows(x: torch.Tensor, what: str) -> torch.Tensor:
    if x.dim() != 2:
        raise ValueError(f"{what} must be (n, dim), got {tuple(x.shape)}")
    if not x.is_cuda:
        raise RuntimeError(f"{what}: the k-NN kernels run on the MI355X only (move the tensor to cuda)")
    return x.to(dtype=torch.float32).contiguous()


def knn_topk(queries: torch.Tensor, bank: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k bank rows of highest dot product for every query row: (sims (Q, k) fp32, idx (Q, k) int64), each row sorted
    by similarity descending, then bank index ascending (NaN similarities come back as -inf).  With l2-normalised rows
    the similarity is the cosine.  Q x N is never materialised."""
    q = _f32_rows(queries, "queries")
    b = q if bank is queries else _f32_rows(bank, "bank")
    Q, D = q.shape
    N = b.shape[0]
    if b.shape[1] != D:
        raise ValueError(f"queries and bank differ in width ({D} vs {b.shape[1]})")
    if not 1 <= k <= min(KNN_MAX_K, N):
        raise ValueError(f"k = {k} outside [1, min({KNN_MAX_K}, bank size {N})]")
    need = lib.mae_knn_scratch_bytes(Q, N, D, k)
    if need < 0:
        raise ValueError(f"k-NN shape outside the kernel's limits (Q {Q}, N {N}, dim {D}, k {k}): dim must be a multiple of 4 in [4, 4096]")
    dev = q.device
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    sims = torch.empty(Q, k, dtype=torch.float32, device=dev)
    idx = torch.empty(Q, k, dtype=torch.int64, device=dev)
    check(lib.mae_knn_topk(_ptr(q), Q, _ptr(b), N, D, k, _ptr(sims), _ptr(idx), _ptr(scratch), need, _stream(dev)))
    return sims, idx


def knn_vote(sims: torch.Tensor, idx: torch.Tensor, bank_labels: torch.Tensor, num_classes: int, k: Optional[int] = None,
             temperature: float = 0.07, return_scores: bool = False, bank_size: Optional[int] = None):
    """Weighted vote over the first ``k`` neighbours (default all): scores[q][c] = sum_j [label(idx_j) == c] exp(sim_j / T);
    returns pred (Q,) int64 (argmax, lowest class among ties; -1 where a neighbour's label is outside [0, num_classes)),
    and the (Q, C) scores first with ``return_scores``.  ``bank_size``: when given, bank_labels must hold exactly that many
    labels (one per bank row)."""
    if sims.shape != idx.shape or sims.dim() != 2:
        raise ValueError(f"sims and idx must be the same (Q, k) shape, got {tuple(sims.shape)} and {tuple(idx.shape)}")
    Q, ks = sims.shape
    k = ks if k is None else int(k)
    if not 1 <= k <= ks:
        raise ValueError(f"k = {k} outside [1, {ks}]")
    if bank_size is not None and bank_labels.numel() != bank_size:
        raise ValueError(f"bank_labels has {bank_labels.numel()} entries for a bank of {bank_size} rows")
    dev = sims.device
    s = sims.to(dtype=torch.float32).contiguous()
    i = idx.to(dtype=torch.int64).contiguous()
    lab = bank_labels.to(device=dev, dtype=torch.int64).contiguous().view(-1)
    # the kernel reads bank_labels[idx] and only knows idx >= 0: an index past the labels is refused here
    if int(i.max()) >= lab.numel():
        raise ValueError(f"a neighbour index ({int(i.max())}) lies past bank_labels ({lab.numel()} entries)")
    pred = torch.empty(Q, dtype=torch.int64, device=dev)
    scores = torch.empty(Q, num_classes, dtype=torch.float32, device=dev) if return_scores else None
    check(lib.mae_knn_vote(_ptr(s), _ptr(i), Q, ks, k, _ptr(lab), int(num_classes), float(temperature), _ptr(scores), _ptr(pred), _stream(dev)))
    return (scores, pred) if return_scores else pred


def knn_classify(bank_feats: torch.Tensor, bank_labels: torch.Tensor, query_feats: torch.Tensor, query_labels: torch.Tensor,
                 ks: Sequence[int] = DEFAULT_KS, temperature: float = 0.07, num_classes: Optional[int] = None) -> Dict[int, float]:
    """Top-1 accuracy of the weighted k-NN classifier for every k in ``ks``: ONE top-k search at max(ks), one vote per k."""
    ks = sorted({int(k) for k in ks})
    if not ks or ks[0] < 1:
        raise ValueError(f"ks must hold positive integers, got {ks}")
    if bank_labels.numel() != bank_feats.shape[0]:
        raise ValueError(f"bank_labels has {bank_labels.numel()} entries for {bank_feats.shape[0]} bank rows")
    if query_labels.numel() != query_feats.shape[0]:
        raise ValueError(f"query_labels has {query_labels.numel()} entries for {query_feats.shape[0]} queries")
    if ks[-1] > bank_feats.shape[0]:
        raise ValueError(f"k = {ks[-1]} exceeds the bank size {bank_feats.shape[0]}")
    C = int(num_classes) if num_classes is not None else int(torch.cat([bank_labels.flatten(), query_labels.flatten()]).max()) + 1
    sims, idx = knn_topk(query_feats, bank_feats, ks[-1])
    y = query_labels.to(device=sims.device, dtype=torch.int64)
    return {k: float((knn_vote(sims, idx, bank_labels, C, k=k, temperature=temperature, bank_size=bank_feats.shape[0]) == y.view(-1)).double().mean())
            for k in ks}


def parse_ks(text: Union[str, Iterable[int]]) -> Tuple[int, ...]:
    """``"10,20,100,200"`` -> (10, 20, 100, 200): sorted, unique, each in [1, 256]."""
    vals = [int(t) for t in text.split(",") if t.strip()] if isinstance(text, str) else [int(t) for t in text]
    if not vals or any(not 1 <= v <= KNN_MAX_K for v in vals):
        raise ValueError(f"--k needs comma-separated integers in [1, {KNN_MAX_K}], got {text!r}")
    return tuple(sorted(set(vals)))


def config_depth_dim(model_cfg: Dict[str, Any]) -> Tuple[int, int]:
    """(depth, embed_dim) of the encoder a ``model`` config section builds, with the defaults of ``MaskedAutoencoder``: what the
    evaluation tools need to check ``--layers`` before anything is loaded."""
    enc = model_cfg.get("encoder", {}) or {}
    return int(enc.get("depth", 12)), int(enc.get("embed_dim", 384))


def parse_layers(spec: str, depth: int) -> Tuple[int, ...]:
    """The ``--layers`` argument of the evaluation tools as block indices of an encoder of ``depth`` blocks, sorted:
    ``"last"`` -> (depth - 1,); ``"lastN"`` -> the last N blocks (``"last4"``: DINO's ViT-S probe); ``"each"`` -> every block (the
    per-layer curve); ``"2,5,-1"`` -> the blocks listed, negative ones from the end.  An unknown word, an index outside the model,
    a repeat, or N outside [1, depth] raises ValueError."""
    text = str(spec).strip().lower()
    if depth < 1:
        raise ValueError(f"depth must be positive, got {depth}")
    if text == "each":
        return tuple(range(depth))
    if text.startswith("last"):
        tail = text[4:]
        if tail and not tail.isdigit():
            raise ValueError(f"--layers {spec!r}: expected last, lastN, each or comma-separated block indices")
        n = int(tail) if tail else 1
        if not 1 <= n <= depth:
            raise ValueError(f"--layers {spec!r}: the encoder has {depth} blocks")
        return tuple(range(depth - n, depth))
    try:
        vals = [int(t) for t in text.split(",")]
    except ValueError:
        raise ValueError(f"--layers {spec!r}: expected last, lastN, each or comma-separated block indices") from None
    if any(not -depth <= v < depth for v in vals):
        raise ValueError(f"--layers {spec!r}: block index outside the encoder's {depth} blocks")
    out = sorted(v + depth if v < 0 else v for v in vals)
    if len(set(out)) != len(out):
        raise ValueError(f"--layers {spec!r}: a block is named twice")
    return tuple(out)


def attention_grid(maps: torch.Tensor, with_cls: bool, grid: int) -> torch.Tensor:
    """Attention maps or a rollout, (..., T) over the keys, as patch grids (..., grid, grid): the class column (the first, with
    ``with_cls``) is dropped, the patch columns are renormalised to sum 1 and laid out row-major as the patches are.  A row whose
    whole mass sits on the class key has no patch map and raises."""
    n = int(grid) * int(grid)
    if grid < 1 or maps.dim() < 1 or maps.shape[-1] != n + (1 if with_cls else 0):
        raise ValueError(f"expected (..., {n + (1 if with_cls else 0)}) keys for a {grid} x {grid} grid (with_cls={bool(with_cls)}), got {tuple(maps.shape)}")
    patches = maps[..., 1:] if with_cls else maps
    total = patches.sum(dim=-1, keepdim=True)
    if not bool((total > 0).all()):
        raise ValueError("a map puts no attention on the patch keys")
    return (patches / total).reshape(*maps.shape[:-1], grid, grid)


# ---------------------------------------------------------------------------------------------------------------------
# normalisation (scripts/evaluation/visualize_representation.py:99-115)
# ---------------------------------------------------------------------------------------------------------------------
def apply_normalization(features, mode: str):
    """none | l2 (rows / (||row|| + 1e-8)) | channel ((x - mean) / (population std + 1e-8) per column): the reference's
    numpy formulas, on a numpy array or a torch tensor."""
    if mode == "none":
        return features
    if isinstance(features, np.ndarray):
        if mode == "l2":
            return features / (np.linalg.norm(features, axis=1, keepdims=True) + 1e-8)
        if mode == "channel":
            return (features - features.mean(axis=0, keepdims=True)) / (features.std(axis=0, keepdims=True) + 1e-8)
    else:
        if mode == "l2":
            return features / (torch.linalg.vector_norm(features, dim=1, keepdim=True) + 1e-8)
        if mode == "channel":
            return (features - features.mean(dim=0, keepdim=True)) / (features.std(dim=0, unbiased=False, keepdim=True) + 1e-8)
    raise ValueError(f"Unknown normalization mode: {mode}")


# ---------------------------------------------------------------------------------------------------------------------
# encoders and checkpoints
# ---------------------------------------------------------------------------------------------------------------------
@dataclass
class EvalEncoder:
    """A frozen encoder ready for feature extraction: ``vit`` (MAE / classifier / random / an I-JEPA ``.pt`` encoder
    loaded into a plain ViT) or ``ijepa`` (an I-JEPA model whose ``encoder`` is "target" or "context")."""
    kind: str                 # "mae" | "classifier" | "ijepa" | "random"
    layout: str               # checkpoint layout (checkpoint_layout) or "random"
    encoder: str              # "vit" | "target" | "context"
    vit: Optional[_ViT] = None
    ijepa: Any = None

    @property
    def with_cls(self) -> bool:
        """False for every encoder trained on the patch tokens alone: I-JEPA, and a classifier fine-tuned from one."""
        return self.kind != "ijepa" and (self.vit is None or bool(self.vit.with_cls))

    @property
    def embed_dim(self) -> int:
        return self.ijepa.embed_dim if self.ijepa is not None else self.vit.embed_dim

    def to(self, device) -> "EvalEncoder":
        if self.ijepa is not None:
            self.ijepa.to(device)
        else:
            self.vit._owner().to(device)
        return self

    @property
    def depth(self) -> int:
        """Number of encoder blocks: what ``layers`` indexes."""
        model = self.ijepa.net if self.ijepa is not None else self.vit._owner()
        return int(model._dims["depth"])

    def features(self, images: torch.Tensor, pool: str = "cls", normalize: str = "none", layers: Optional[Sequence[int]] = None) -> torch.Tensor:
        """(B, D) pooled features of the last block, or with ``layers`` (block indices, ascending) (B, n, W) from one forward pass:
        see ``MaskedAutoencoder.extract_features``.  normalize="l2" normalises every (layer, pool) slice on its own: the cosine
        similarity of two flattened rows is then the mean of their per-slice cosines."""
        if self.ijepa is not None:
            return self.ijepa.extract_features(images, encoder=self.encoder, pool=pool, normalize=normalize, layers=layers)
        return self.vit.extract_features(images, pool=pool, normalize=normalize, with_cls=self.with_cls, layers=layers)

    def tokens(self, images: torch.Tensor, drop_cls: bool = True) -> torch.Tensor:
        """Every token after the final LayerNorm, (B, T, D) fp32: the patch rows, and with ``drop_cls=False`` the class row in front of
        them where the encoder has one."""
        if self.ijepa is not None:
            return self.ijepa.extract_tokens(images, encoder=self.encoder)
        return self.vit.extract_tokens(images, with_cls=self.with_cls, drop_cls=drop_cls)

    def attention(self, images: torch.Tensor, layers: Sequence[int] = (-1,), query: Optional[str] = None, rollout: bool = False):
        """Attention maps (B, n, H, T) fp32 of the blocks ``layers`` and, with ``rollout``, the (B, T) rollout behind them: see
        ``MaskedAutoencoder.extract_attention``.  query defaults to "cls" where the encoder has a class token, else "mean"."""
        query = ("cls" if self.with_cls else "mean") if query is None else query
        if self.ijepa is not None:
            return self.ijepa.extract_attention(images, encoder=self.encoder, layers=layers, query=query, rollout=rollout)
        return self.vit.extract_attention(images, layers=layers, query=query, with_cls=self.with_cls, rollout=rollout)

    @property
    def num_heads(self) -> int:
        model = self.ijepa.net if self.ijepa is not None else self.vit._owner()
        return int(model._dims["num_heads"])


def checkpoint_layout(state: Dict[str, Any]) -> str:
    """Which of the five known layouts a state dict has: ``mae_ckpt`` (MAE Lightning, model.encoder.vit.*), ``classifier_ckpt``
    (model.encoder.<timm name>), ``mae_pt`` (vit-mae.pt, encoder.vit.*), ``ijepa_ckpt`` (I-JEPA Lightning, model.net.* +
    model.target_arena), ``ijepa_pt`` (vit-ijepa.pt, encoder.vit.* + target_encoder.vit.*).  Raises on anything else."""
    keys = list(state.keys())
    has = lambda pfx: any(k.startswith(pfx) for k in keys)  # noqa: E731
    if has("model.net.encoder.vit.") and "model.target_arena" in state:
        return "ijepa_ckpt"
    if has("model.encoder.vit."):
        return "mae_ckpt"
    if has("target_encoder.vit.") and has("encoder.vit."):
        return "ijepa_pt"
    if has("encoder.vit."):
        return "mae_pt"
    if has("model.encoder.blocks.") or has("model.encoder.cls_token"):
        return "classifier_ckpt"
    raise ValueError("no encoder tensors found: expected model.encoder.vit.* (MAE checkpoint), model.encoder.<timm name> (classifier), "
                     "encoder.vit.* (vit-mae.pt / vit-ijepa.pt) or model.net.* + model.target_arena (I-JEPA checkpoint)")


def _load_vit(vit: _ViT, state: Dict[str, Any], prefix: str) -> None:
    sub = {k[len(prefix):]: v for k, v in state.items() if k.startswith(prefix)}
    expected = list(vit.state_dict().keys())
    missing = [k for k in expected if k not in sub]
    if not sub or missing:
        raise ValueError(f"checkpoint lacks encoder tensors under {prefix!r}: missing {missing[:5]}{' ...' if len(missing) > 5 else ''}")
    with torch.no_grad():
        vit.load_state_dict({k: sub[k] for k in expected}, strict=True)


def _general(model_cfg: Dict[str, Any], precision: Optional[str]) -> Dict[str, Any]:
    cfg = dict(model_cfg)
    g = dict(cfg.get("general", {}))
    if precision is not None:
        g["engine_precision"] = precision
    cfg["general"] = g
    return cfg


def _open_checkpoint(src: Union[str, Path, Dict[str, Any]]) -> Tuple[Any, Dict[str, Any], str]:
    """(checkpoint, state dict, layout) of a path, a loaded checkpoint or a state dict."""
    ckpt = torch.load(src, map_location="cpu", weights_only=False) if isinstance(src, (str, Path)) else src
    state = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
    return ckpt, state, checkpoint_layout(state)


def _ijepa_model(cfg: Dict[str, Any], state: Dict[str, Any]):
    """The ``IJEPA`` model an ``ijepa_ckpt`` state dict loads into; model.predictor in the config fixes the arena layout."""
    from .jepa import IJEPAPretrainModule
    if "predictor" not in cfg:
        raise ValueError("an I-JEPA checkpoint needs model.predictor in the config")
    module = IJEPAPretrainModule(cfg, {})
    module.load_checkpoint_dict({"state_dict": state})
    return module.model


def load_eval_encoder(src: Union[str, Path, Dict[str, Any]], model_cfg: Dict[str, Any], encoder: str = "target",
                      precision: Optional[str] = None, device=None) -> EvalEncoder:
    """The frozen encoder of a checkpoint (a path, a loaded checkpoint or a state dict), or ``"random"`` for the randomly
    initialised baseline ViT (the chance-level reference).  ``encoder`` picks the I-JEPA encoder ("target" = the EMA
    encoder I-JEPA evaluates, or "context"); MAE-family checkpoints ignore it.  Raises when no encoder tensor is found
    or when any is missing (no strict=False fallback)."""
    if encoder not in ("target", "context"):
        raise ValueError(f"encoder must be 'target' or 'context', got {encoder!r}")
    cfg = _general(model_cfg, precision)
    if isinstance(src, str) and src == "random":
        out = EvalEncoder("random", "random", "vit", vit=build_baseline_encoder(cfg, seed=73))
        return out.to(device) if device is not None else out
    ckpt, state, layout = _open_checkpoint(src)
    if layout == "ijepa_ckpt":
        out = EvalEncoder("ijepa", layout, encoder, ijepa=_ijepa_model(cfg, state))
    else:
        vit = encoder_mae(cfg).encoder.vit
        if layout == "ijepa_pt":
            _load_vit(vit, state, "target_encoder.vit." if encoder == "target" else "encoder.vit.")
            vit.with_cls = False
            out = EvalEncoder("ijepa", layout, encoder, vit=vit)
        else:
            prefix = {"mae_ckpt": "model.encoder.vit.", "mae_pt": "encoder.vit.", "classifier_ckpt": "model.encoder."}[layout]
            _load_vit(vit, state, prefix)
            if layout == "classifier_ckpt":  # a classifier fine-tuned from I-JEPA keeps running on the patch tokens alone
                vit.with_cls = checkpoint_with_cls(ckpt)
            out = EvalEncoder("classifier" if layout == "classifier_ckpt" else "mae", layout, "vit", vit=vit)
    return out.to(device) if device is not None else out


def load_ijepa_encoder(src: Union[str, Path, Dict[str, Any]], model_cfg: Dict[str, Any], encoder: str = "target",
                       precision: Optional[str] = None) -> _ViT:
    """An I-JEPA checkpoint as the classifier's encoder node (``ViTClassifier(pretrained_encoder=...)``): a fresh ViT of
    ``model_cfg`` holding the EMA target encoder (``encoder="target"``, what I-JEPA evaluates) or the context encoder, with
    ``with_cls = False`` so that the classifier runs over the patch tokens alone.  Accepts the ``ijepa_ckpt`` layout
    (model.net.* + model.target_arena; needs model.predictor in the config, which fixes the arena layout) and ``ijepa_pt``
    (encoder.vit.* + target_encoder.vit.*).  Strict: any other layout, or a missing encoder tensor, raises."""
    if encoder not in ("target", "context"):
        raise ValueError(f"encoder must be 'target' or 'context', got {encoder!r}")
    cfg = _general(model_cfg, precision)
    _, state, layout = _open_checkpoint(src)
    if layout == "ijepa_ckpt":
        model = _ijepa_model(cfg, state)
        source, prefix = model.target_state_dict() if encoder == "target" else model.net.state_dict(), "encoder.vit."
    elif layout == "ijepa_pt":
        source, prefix = state, "target_encoder.vit." if encoder == "target" else "encoder.vit."
    else:
        raise ValueError(f"not an I-JEPA checkpoint (layout {layout}): expected model.net.* + model.target_arena, or encoder.vit.* + target_encoder.vit.*")
    vit = encoder_mae({k: v for k, v in cfg.items() if k != "decoder"}).encoder.vit  # the classifier never runs a decoder: the smallest one
    _load_vit(vit, source, prefix)
    vit.with_cls = False
    return vit


def _collect_split(batches, fn, max_samples: Optional[int]) -> Tuple[torch.Tensor, torch.Tensor]:
    """fn(images) of every batch of a ``LabeledBatches`` split and its labels (n,) int64, on the device, in the split's order."""
    outs, labels, n = [], [], 0
    for imgs, lbls in batches():
        outs.append(fn(imgs))
        labels.append(lbls)
        n += imgs.shape[0]
        if max_samples is not None and n >= max_samples:
            break
    x, y = torch.cat(outs), torch.cat(labels)
    if max_samples is not None:
        x, y = x[:max_samples], y[:max_samples]
    return x, y


@torch.no_grad()
def extract_split_features(enc: EvalEncoder, batches, pool: str = "cls", normalize: str = "none",
                           max_samples: Optional[int] = None, layers: Optional[Sequence[int]] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Features (n, D) fp32 -- with ``layers`` (n, len(layers), W), see ``EvalEncoder.features`` -- and labels (n,) int64 of a
    ``LabeledBatches`` split, on the device, in the split's order."""
    return _collect_split(batches, lambda imgs: enc.features(imgs, pool=pool, normalize=normalize, layers=layers), max_samples)


@torch.no_grad()
def extract_split_tokens(enc: EvalEncoder, batches, drop_cls: bool = True, max_samples: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Tokens (n, T, D) fp32 and labels (n,) int64 of a ``LabeledBatches`` split, on the device, in the split's order: the cache an
    attentive probe trains on (n T D 4 bytes: 442 MB for 2000 ViT-S/8 images)."""
    return _collect_split(batches, lambda imgs: enc.tokens(imgs, drop_cls=drop_cls), max_samples)
