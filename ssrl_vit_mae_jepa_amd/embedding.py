"""Exact t-SNE of encoder features on the MI355X (k_tsne.hip): ``DeviceTSNE`` and ``pca_init``.

The arithmetic is the library's (``mae_tsne_affinities``, ``mae_tsne_step``); this module holds the buffers and the schedule, which is
sklearn 1.7's ``TSNE``: learning rate "auto" = max(n / early_exaggeration / 4, 50); momentum 0.5 and exaggeration 12 for the first 250
iterations, then momentum 0.8 and exaggeration 1; gains +0.2 / x0.8 clamped below at ``min_gain``.

Two deviations from ``sklearn.manifold.TSNE``, both on purpose:
  * the gradient is exact, not Barnes-Hut (sklearn's default ``method="barnes_hut"`` with ``angle=0.5``): every one of the n^2 pairs
    is summed, there is no approximation parameter, and n <= 16384;
  * there is no early stopping on the gradient norm or on stalled progress (sklearn's ``min_grad_norm`` / ``n_iter_without_progress``):
    that needs a host round trip every 50 iterations, and here nothing synchronises inside the loop.  ``max_iter`` iterations run.
The KL divergence (of the unexaggerated P) is written into a device buffer every ``kl_every`` iterations and after the last, and read
once at the end.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import check, lib
from .mae import _ptr, _stream

MIN_N, MAX_N, MAX_DIM = 8, 16384, 8192   # the limits of k_tsne.hip


def check_limits(n: int, dim: int, perplexity: float) -> None:
    """Raise ValueError naming the limit that (n, dim, perplexity) breaks: the library's own limits, checked before any buffer exists."""
    if not MIN_N <= n <= MAX_N:
        raise ValueError(f"DeviceTSNE: n = {n} outside [{MIN_N}, {MAX_N}]")
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"DeviceTSNE: dim = {dim} outside [1, {MAX_DIM}]")
    if not 1.0 <= perplexity < n - 1:
        raise ValueError(f"DeviceTSNE: perplexity = {perplexity:g} outside [1, n - 1 = {n - 1})")


def pca_init(features) -> np.ndarray:
    """(n, 2) fp32: the top two principal components of the rows, in float64 numpy on the host, scaled so that the first has standard
    deviation 1e-4 (sklearn's init="pca").  The sign of a component is the SVD's: a flip mirrors the map and changes nothing else."""
    x = np.asarray(features.detach().cpu() if isinstance(features, torch.Tensor) else features, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2 or x.shape[1] < 2:
        raise ValueError(f"pca_init: features must be (n >= 2, dim >= 2), got {x.shape}")
    x = x - x.mean(0, keepdims=True)
    if x.shape[1] <= x.shape[0]:
        _, vec = np.linalg.eigh(x.T @ x)              # ascending eigenvalues: the last two columns
        z = x @ vec[:, [-1, -2]]
    else:
        val, vec = np.linalg.eigh(x @ x.T)
        z = vec[:, [-1, -2]] * np.sqrt(np.maximum(val[[-1, -2]], 0.0))
    return (z / np.std(z[:, 0]) * 1e-4).astype(np.float32)


def schedule(iteration: int, n: int, early_exaggeration: float = 12.0, exaggeration_iters: int = 250, learning_rate="auto") -> Dict[str, float]:
    """momentum, exaggeration and learning rate of iteration ``iteration`` (from 0)."""
    lr = max(n / early_exaggeration / 4.0, 50.0) if learning_rate == "auto" else float(learning_rate)
    early = iteration < exaggeration_iters
    return dict(momentum=0.5 if early else 0.8, alpha=float(early_exaggeration) if early else 1.0, learning_rate=lr)


class DeviceTSNE:
    def __init__(self, perplexity: float = 30.0, max_iter: int = 1000, early_exaggeration: float = 12.0, exaggeration_iters: int = 250,
                 learning_rate="auto", min_gain: float = 0.01, kl_every: int = 50):
        if max_iter < 1 or kl_every < 1 or exaggeration_iters < 0:
            raise ValueError("DeviceTSNE: max_iter and kl_every must be >= 1, exaggeration_iters >= 0")
        self.perplexity, self.max_iter, self.early_exaggeration = float(perplexity), int(max_iter), float(early_exaggeration)
        self.exaggeration_iters, self.learning_rate, self.min_gain, self.kl_every = int(exaggeration_iters), learning_rate, float(min_gain), int(kl_every)
        self.n = 0
        self.iteration = 0

    # ---- state ------------------------------------------------------------------------------------------------------------
    def prepare(self, features: torch.Tensor, init, outputs: bool = False) -> "DeviceTSNE":
        """Compute P from features (n, dim) on the device and set y = init (n, 2), update = 0, gains = 1, iteration = 0.
        outputs: also keep sqdist, beta and p_cond (the tests read them)."""
        if features.dim() != 2:
            raise ValueError(f"DeviceTSNE: features must be (n, dim), got {tuple(features.shape)}")
        n, dim = features.shape
        check_limits(n, dim, self.perplexity)
        if not features.is_cuda:
            raise RuntimeError("DeviceTSNE works on device tensors only (no CPU fallback); move the features to cuda")
        dev = features.device
        x = features.detach().to(torch.float32).contiguous()
        y = torch.as_tensor(init, dtype=torch.float32).to(dev).contiguous().clone()
        if tuple(y.shape) != (n, 2):
            raise ValueError(f"DeviceTSNE: init must be ({n}, 2), got {tuple(y.shape)}")
        pitch = lib.mae_tsne_pitch(n)
        self.n, self.pitch, self.device = n, pitch, dev
        self.P = torch.empty((n, pitch), dtype=torch.float32, device=dev)
        self.sqdist = torch.empty((n, n), dtype=torch.float32, device=dev) if outputs else None
        self.p_cond = torch.empty((n, n), dtype=torch.float32, device=dev) if outputs else None
        self.beta = torch.empty(n, dtype=torch.float32, device=dev)
        check(lib.mae_tsne_affinities(_ptr(x), n, dim, self.perplexity, _ptr(self.P), _ptr(self.sqdist), _ptr(self.beta), _ptr(self.p_cond), _stream(dev)))
        self.y = y
        self.update = torch.zeros_like(y)
        self.gains = torch.ones_like(y)
        self.grad = torch.zeros_like(y)
        self.scratch = torch.empty(lib.mae_tsne_scratch_bytes(n, dim), dtype=torch.uint8, device=dev)
        slots = self.max_iter // self.kl_every + 2
        self.kl_buffer = torch.zeros(slots, dtype=torch.float32, device=dev)
        self.kl_iterations = []          # the iteration count after which slot k was written
        self.iteration = 0
        return self

    def step(self, k: int = 1) -> "DeviceTSNE":
        """Advance k iterations; y, update, gains, grad (of the last iteration) and iteration stay readable.  No host synchronisation."""
        if self.n == 0:
            raise RuntimeError("DeviceTSNE.step before prepare")
        s = _stream(self.device)
        for _ in range(int(k)):
            sch = schedule(self.iteration, self.n, self.early_exaggeration, self.exaggeration_iters, self.learning_rate)
            done = self.iteration + 1
            kl = None
            if (done % self.kl_every == 0 or done == self.max_iter) and len(self.kl_iterations) < self.kl_buffer.numel():
                kl = self.kl_buffer[len(self.kl_iterations):len(self.kl_iterations) + 1]
                self.kl_iterations.append(done)
            # the KL value is the one of the embedding the gradient was taken at: y before this iteration's step
            check(lib.mae_tsne_step(_ptr(self.P), _ptr(self.y), _ptr(self.update), _ptr(self.gains), self.n, sch["alpha"], sch["momentum"],
                                    sch["learning_rate"], self.min_gain, _ptr(self.grad), _ptr(kl), _ptr(self.scratch), self.scratch.numel(), s))
            self.iteration = done
        return self

    def kl_divergence(self) -> torch.Tensor:
        """One device float: the KL divergence of the current y (a gradient pass; nothing is stepped)."""
        out = torch.empty(1, dtype=torch.float32, device=self.device)
        g = torch.empty_like(self.grad)
        check(lib.mae_tsne_gradient(_ptr(self.P), _ptr(self.y), self.n, 1.0, _ptr(g), _ptr(out), _ptr(self.scratch), self.scratch.numel(), _stream(self.device)))
        return out

    def fit(self, features: torch.Tensor, init: Optional[object] = None) -> Tuple[torch.Tensor, Dict]:
        """-> (Z (n, 2) fp32 on the device, info).  init None = pca_init(features).  info: n, iterations, perplexity, learning_rate,
        kl_trace = [[iteration, KL of the embedding that iteration started from], ...] and kl_divergence of the final embedding."""
        init = pca_init(features) if init is None else init
        self.prepare(features, init)
        self.step(self.max_iter)
        final = self.kl_divergence()
        trace = self.kl_buffer[:len(self.kl_iterations)].cpu().tolist()   # the one read
        info = dict(n=self.n, iterations=self.iteration, perplexity=self.perplexity,
                    learning_rate=schedule(0, self.n, self.early_exaggeration, self.exaggeration_iters, self.learning_rate)["learning_rate"],
                    kl_trace=[[it, v] for it, v in zip(self.kl_iterations, trace)], kl_divergence=float(final.item()))
        return self.y, info
