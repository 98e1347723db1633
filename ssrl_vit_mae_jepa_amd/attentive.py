"""Attentive probing on cached patch tokens: the frozen-encoder evaluation of the JEPA line of work (V-JEPA; AIM before it).

One learned query cross-attends over the frozen encoder's tokens, a linear layer classifies the pooled vector:
``BatchNorm1d(D, affine=False, eps=1e-6)`` over all token rows, keys and values ``xh Wk^T`` / ``xh Wv^T`` without bias, one query
``q`` split over the heads, softmax over the tokens, then ``ProbeHead``'s linear layer.  The encoder is frozen, so the tokens are
extracted once (``representation.extract_split_tokens``) and every epoch runs over the cache.

``AttentiveProbe.step`` is native end to end and never writes anything of the size of the tokens: ``mae_batchnorm_stats``,
``mae_attn_probe_fold``, ``mae_attn_pool_fwd`` (one read of the tokens), ``mae_attn_probe_project``, ``mae_classifier_head`` on the
pooled rows (fp32, seq_len 1, the class-row pool; its d_feats is dp), ``mae_attn_probe_project_bwd``, ``mae_attn_pool_bwd`` (the
second read), ``mae_attn_probe_fold_bwd`` and the buffer AdamW (``mae_engine_adamw_buffer``) with weight decay on the three matrices
only and no clipping.  Nothing synchronises with the host.

The hyper-parameter defaults are this tool's own (a learning rate of 1e-3 x batch / 256, weight decay 0.05, 90 epochs with 10 of
warm-up); they are not a paper's recipe.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch

from ._lib import check, lib
from .classifier import MAX_CLASSES, _pad4, _trunc_normal
from .mae import Engine, _ptr, _stream
from .probe import _Probe, parse_block, probe_lr

ATTENTIVE_DEFAULTS: Dict[str, Any] = {
    "total_epochs": 90, "warmup_epochs": 10, "batch_size": 256, "base_learning_rate": 1e-3, "weight_decay": 0.05, "heads": None,
    "tokens": "patches", "bn_eps": 1e-6, "bn_momentum": 0.1, "init_std": 0.02, "head_init_std": 0.01, "beta1": 0.9, "beta2": 0.999,
    "adam_eps": 1e-8}
TOKEN_SETS = ("patches", "all")
MAX_HEADS = 16


def parse_attentive_probe(block: Optional[Dict[str, Any]]) -> Dict[str, Any]:
    """The YAML block ``attentive_probe:`` checked and completed with ``ATTENTIVE_DEFAULTS``; an unknown key is refused by name.
    ``heads: null`` means the encoder's head count (the caller fills it in)."""
    out = parse_block(block, ATTENTIVE_DEFAULTS, "attentive_probe", ("total_epochs", "warmup_epochs", "batch_size"),
                      ("base_learning_rate", "weight_decay", "bn_eps", "bn_momentum", "init_std", "head_init_std", "beta1", "beta2", "adam_eps"))
    if out["heads"] is not None:
        out["heads"] = int(out["heads"])
        if not 1 <= out["heads"] <= MAX_HEADS:
            raise ValueError(f"attentive_probe.heads must be in [1, {MAX_HEADS}], got {out['heads']}")
    if out["tokens"] not in TOKEN_SETS:
        raise ValueError(f"attentive_probe.tokens must be one of {list(TOKEN_SETS)}, got {out['tokens']!r}")
    if out["total_epochs"] < 1 or out["warmup_epochs"] < 0 or out["batch_size"] < 1:
        raise ValueError("attentive_probe: total_epochs >= 1, warmup_epochs >= 0 and batch_size >= 1")
    if not (out["base_learning_rate"] > 0 and out["weight_decay"] >= 0 and 0 <= out["beta1"] < 1 and 0 <= out["beta2"] < 1 and out["adam_eps"] > 0):
        raise ValueError("attentive_probe: base_learning_rate > 0, weight_decay >= 0, beta1 and beta2 in [0, 1), adam_eps > 0")
    if not (out["bn_eps"] >= 0 and 0 <= out["bn_momentum"] <= 1 and out["init_std"] > 0 and out["head_init_std"] > 0):
        raise ValueError("attentive_probe: bn_eps >= 0, bn_momentum in [0, 1], init_std > 0, head_init_std > 0")
    return out


attentive_lr = probe_lr   # the peak learning rate: base_learning_rate * batch_size / 256


def layout(dim: int, num_classes: int) -> Dict[str, Tuple[int, int]]:
    """name -> (offset, count) inside the flat parameter buffer: q | Wk | Wv | W | b (+ padding to a multiple of 4 floats)."""
    d2 = dim * dim
    out, off = {}, 0
    for name, n in (("q", dim), ("wk", d2), ("wv", d2), ("w", num_classes * dim), ("b", num_classes)):
        out[name] = (off, n)
        off += n
    out["total"] = (0, _pad4(off))
    return out


# the buffer AdamW lives behind an engine handle (it feeds the engine's timers); the smallest engine there is serves every probe
_OPT_ENGINE: Optional[Engine] = None


def _opt_engine() -> Engine:
    global _OPT_ENGINE
    if _OPT_ENGINE is None:
        _OPT_ENGINE = Engine(dict(image_size=8, patch_size=4, in_chans=3, embed_dim=16, depth=1, num_heads=1, decoder_embed_dim=16, decoder_depth=1,
                                  decoder_num_heads=1), "fp32")
    return _OPT_ENGINE


class AttentiveProbe(_Probe):
    """The probe's state (one flat fp32 parameter buffer, the BatchNorm running statistics, the AdamW moments, gradient and scratch
    buffers) and its operations.  ``cfg``: a ``parse_attentive_probe`` result (or a subset of its keys); tokens are (B, T, dim) fp32 on
    the device."""

    def __init__(self, dim: int, num_classes: int, heads: int, cfg: Optional[Dict[str, Any]] = None, seed: Optional[int] = 73, device=None):
        self.cfg = parse_attentive_probe(cfg)
        dim, num_classes, heads = int(dim), int(num_classes), int(heads)
        if dim % 4 != 0 or not 4 <= dim <= 1024:
            raise ValueError(f"the attentive probe needs a token width that is a multiple of 4 in [4, 1024], got {dim}")
        if not 1 <= heads <= MAX_HEADS or dim % heads != 0:
            raise ValueError(f"heads must be in [1, {MAX_HEADS}] and divide the token width {dim}, got {heads}")
        if not 2 <= num_classes <= MAX_CLASSES:
            raise ValueError(f"num_classes must be in [2, {MAX_CLASSES}], got {num_classes}")
        self.dim, self.num_classes, self.heads = dim, num_classes, heads
        self.cfg["heads"] = heads
        self.layout = layout(dim, num_classes)
        n = self.layout["total"][1]
        self.flat = torch.zeros(n, dtype=torch.float32)
        g = torch.Generator().manual_seed(seed) if seed is not None else None
        std = self.cfg["init_std"]
        self.q.copy_(torch.randn(dim, generator=g) * std)
        self.wk.copy_(torch.randn(dim, dim, generator=g) * std)
        self.wv.copy_(torch.randn(dim, dim, generator=g) * std)
        self.w.copy_(_trunc_normal((num_classes, dim), self.cfg["head_init_std"], g))
        self.grads = torch.zeros(n, dtype=torch.float32)     # the same layout; the padding stays zero
        self.exp_avg, self.exp_avg_sq = torch.zeros(n, dtype=torch.float32), torch.zeros(n, dtype=torch.float32)
        self.running_mean, self.running_var = torch.zeros(dim, dtype=torch.float32), torch.ones(dim, dtype=torch.float32)
        self.num_batches_tracked = 0
        self.steps = 0
        self.epoch = 0
        self._scratch: Dict[str, torch.Tensor] = {}
        self.last: Dict[str, torch.Tensor] = {}              # mean, rstd, uq, ybar, lse, p, logits of the latest call (the tests read them)
        if device is not None:
            self.to(device)

    # ---- views into the flat buffers ---------------------------------------------------------------------------
    def _view(self, buf: torch.Tensor, name: str) -> torch.Tensor:
        off, n = self.layout[name]
        shape = {"q": (self.dim,), "wk": (self.dim, self.dim), "wv": (self.dim, self.dim), "w": (self.num_classes, self.dim), "b": (self.num_classes,)}[name]
        return buf[off:off + n].view(shape)

    q = property(lambda self: self._view(self.flat, "q"))
    wk = property(lambda self: self._view(self.flat, "wk"))
    wv = property(lambda self: self._view(self.flat, "wv"))
    w = property(lambda self: self._view(self.flat, "w"))
    b = property(lambda self: self._view(self.flat, "b"))

    def grad(self, name: str) -> torch.Tensor:
        return self._view(self.grads, name)

    @property
    def head_flat(self) -> torch.Tensor:
        """W then b (+ padding): the buffer mae_classifier_head reads."""
        return self.flat[self.layout["w"][0]:]

    def to(self, device) -> "AttentiveProbe":
        for k in ("flat", "grads", "exp_avg", "exp_avg_sq", "running_mean", "running_var"):
            setattr(self, k, getattr(self, k).to(device))
        self._scratch.clear()
        return self

    @property
    def device(self) -> torch.device:
        return self.flat.device

    _INPUT = ("the attentive probe's", "AttentiveProbe", "tokens", ("B", "T"), "images")

    # ---- the forward pass ----------------------------------------------------------------------------------------
    def _statistics(self, tokens: torch.Tensor, training: bool) -> Tuple[torch.Tensor, torch.Tensor]:
        D = tokens.shape[2]
        mean, rstd = self._f32("mean", D), self._f32("rstd", D)
        self._batchnorm(tokens, self.running_mean, self.running_var, training, mean, rstd)
        return mean, rstd

    def _forward(self, tokens: torch.Tensor, labels: Optional[torch.Tensor], training: bool):
        B, T, D = tokens.shape
        H, s = self.heads, _stream(tokens.device)
        mean, rstd = self._statistics(tokens, training)
        uq, ybar, lse, p = self._f32("uq", H, D), self._f32("ybar", B, H, D), self._f32("lse", B, H), self._f32("p", B, D)
        check(lib.mae_attn_probe_fold(_ptr(self.q), _ptr(self.wk), _ptr(rstd), D, H, _ptr(uq), s))
        check(lib.mae_attn_pool_fwd(_ptr(tokens), _ptr(mean), _ptr(uq), B, T, D, H, _ptr(ybar), _ptr(lse), s))
        check(lib.mae_attn_probe_project(_ptr(ybar), _ptr(rstd), _ptr(self.wv), B, D, H, _ptr(p), s))
        dp = self._f32("dp", B, D) if training else None
        head_grads = self.grads[self.layout["w"][0]:] if training else None
        logits, loss, correct = self._classifier_head(p, self.head_flat, labels, head_grads, dp)
        self.last = dict(mean=mean, rstd=rstd, uq=uq, ybar=ybar, lse=lse, p=p, logits=logits)
        return logits, loss, correct, dp

    # ---- the operations ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def loss_and_grads(self, tokens: torch.Tensor, labels: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """Forward in training mode (batch statistics, the running buffers updated) and backward into ``grads``; no optimizer step.
        (loss (1,) fp32, correct (1,) int32), device tensors."""
        tokens, labels = self._check(tokens, labels)
        B, T, D = tokens.shape
        if B * T < 2:
            raise ValueError("a probe step needs at least 2 token rows (BatchNorm in training mode)")
        H, dev = self.heads, tokens.device
        s = _stream(dev)
        logits, loss, correct, dp = self._forward(tokens, labels, True)
        self.num_batches_tracked += 1
        L = self.last
        g, duq = self._f32("g", B, H, D), self._f32("duq", H, D)
        need = lib.mae_attn_probe_project_bwd_scratch_bytes(B, D, H)
        sc = self._bytes("wv", need)
        check(lib.mae_attn_probe_project_bwd(_ptr(dp), _ptr(L["ybar"]), _ptr(L["rstd"]), _ptr(self.wv), B, D, H, _ptr(g), _ptr(self.grad("wv")),
                                             _ptr(sc), sc.numel(), s))
        need = lib.mae_attn_pool_bwd_scratch_bytes(B, T, D, H)
        if need < 0:
            raise ValueError(f"token shape ({B}, {T}, {D}) with {H} heads outside the kernel's limits")
        sc = self._bytes("pool", need)
        check(lib.mae_attn_pool_bwd(_ptr(tokens), _ptr(L["mean"]), _ptr(L["uq"]), _ptr(L["lse"]), _ptr(L["ybar"]), _ptr(g), B, T, D, H, _ptr(duq),
                                    _ptr(sc), sc.numel(), s))
        check(lib.mae_attn_probe_fold_bwd(_ptr(duq), _ptr(self.q), _ptr(self.wk), _ptr(L["rstd"]), D, H, _ptr(self.grad("q")), _ptr(self.grad("wk")), s))
        return loss, correct

    @torch.no_grad()
    def step(self, tokens: torch.Tensor, labels: torch.Tensor, lr: float) -> Tuple[torch.Tensor, torch.Tensor]:
        """One training step: ``loss_and_grads`` then AdamW (weight decay on Wk, Wv and W only, no clipping).  No synchronisation."""
        loss, correct = self.loss_and_grads(tokens, labels)
        self.steps += 1
        c, dev = self.cfg, self.device
        stats = self._scratch.get("stats")
        if stats is None or stats.device != dev:
            stats = self._scratch["stats"] = torch.tensor([0.0, 1.0, 0.0, 0.0], dtype=torch.float32, device=dev)   # [1]: the clip coefficient
        h = _opt_engine().handle
        lo_m, hi_m = self.layout["wk"][0], self.layout["b"][0]        # Wk | Wv | W are contiguous
        for lo, hi, wd in ((0, lo_m, 0.0), (lo_m, hi_m, c["weight_decay"]), (hi_m, self.flat.numel(), 0.0)):
            check(lib.mae_engine_adamw_buffer(h, _ptr(self.flat[lo:hi]), _ptr(self.grads[lo:hi]), _ptr(self.exp_avg[lo:hi]), _ptr(self.exp_avg_sq[lo:hi]),
                                              hi - lo, float(lr), c["beta1"], c["beta2"], c["adam_eps"], float(wd), self.steps, _ptr(stats), _stream(dev)))
        return loss, correct

    @torch.no_grad()
    def evaluate(self, tokens: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """(logits, loss or None, correct or None) with the running statistics; changes no state."""
        tokens, labels = self._check(tokens, labels)
        logits, loss, correct, _ = self._forward(tokens, labels, False)
        return logits, loss, correct

    # ---- resume ----------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        out = {k: getattr(self, k).detach().cpu().clone() for k in ("flat", "exp_avg", "exp_avg_sq", "running_mean", "running_var")}
        out.update(num_batches_tracked=int(self.num_batches_tracked), steps=int(self.steps), epoch=int(self.epoch), cfg=dict(self.cfg), dim=self.dim,
                   num_classes=self.num_classes, heads=self.heads)
        return out

    @torch.no_grad()
    def load_state_dict(self, state: Dict[str, Any]) -> None:
        for k in ("dim", "num_classes", "heads"):
            if int(state[k]) != getattr(self, k):
                raise ValueError(f"the state has {k} = {state[k]}, the probe {getattr(self, k)}")
        for k in ("flat", "exp_avg", "exp_avg_sq", "running_mean", "running_var"):
            dst = getattr(self, k)
            if state[k].numel() != dst.numel():
                raise ValueError(f"{k} has {state[k].numel()} elements, the probe {dst.numel()}")
            dst.copy_(state[k].to(dst.device))
        self.num_batches_tracked, self.steps, self.epoch = int(state["num_batches_tracked"]), int(state["steps"]), int(state["epoch"])
