"""Exact t-SNE and UMAP of encoder features on the MI355X (k_tsne.hip, k_umap.hip): ``DeviceTSNE``, ``DeviceUMAP``.

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

``DeviceUMAP`` (k_umap.hip) is UMAP (McInnes et al.) with umap-learn 0.5's defaults: exact neighbours and umap-learn's
smooth distances from ``mae_umap_fuzzy_knn``, the fuzzy union assembled once with torch ops on the device (``fuzzy_graph``), the curve
(a, b) fitted on the host (``find_ab_params``), the top two principal components scaled to 10 as the start (``umap_init``; spectral
initialisation is left out), and ``mae_umap_epoch`` once per epoch.  Two deviations from ``umap.UMAP``, both on purpose:
  * the layout update is synchronous (Jacobi): every row of epoch t is formed from the positions as the epoch started and written to a
    second buffer, where umap-learn's SGD updates in place while other threads read (and is not reproducible across runs with more
    than one thread).  Here two fits give the same bits, with no atomics.  An edge (i, j) moves row i twice, as the head of (i, j) and
    as the tail of (j, i): umap-learn's ``move_other`` on a symmetric edge list;
  * every firing of an edge draws ``negative_sample_rate`` negative samples, a constant, where umap-learn draws the running quotient
    (epoch - next_negative) / epochs_per_negative_sample, which averages to the same number.
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


def _principal_pair(features, who: str) -> np.ndarray:
    """(n, 2) float64: the rows' coordinates on their top two principal components, in float64 numpy on the host.  The sign of a
    component is the SVD's: a flip mirrors the map and changes nothing else."""
    x = np.asarray(features.detach().cpu() if isinstance(features, torch.Tensor) else features, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2 or x.shape[1] < 2:
        raise ValueError(f"{who}: features must be (n >= 2, dim >= 2), got {x.shape}")
    x = x - x.mean(0, keepdims=True)
    if x.shape[1] <= x.shape[0]:
        _, vec = np.linalg.eigh(x.T @ x)              # ascending eigenvalues: the last two columns
        return x @ vec[:, [-1, -2]]
    val, vec = np.linalg.eigh(x @ x.T)
    return vec[:, [-1, -2]] * np.sqrt(np.maximum(val[[-1, -2]], 0.0))


def pca_init(features) -> np.ndarray:
    """(n, 2) fp32: the top two principal components of the rows, scaled so that the first has standard deviation 1e-4 (sklearn's
    init="pca")."""
    z = _principal_pair(features, "pca_init")
    return (z / np.std(z[:, 0]) * 1e-4).astype(np.float32)


def umap_init(features) -> np.ndarray:
    """(n, 2) fp32: the top two principal components of the rows, scaled so that the largest |coordinate| is 10 (the scale umap-learn
    gives its initialisations).  No noise is added."""
    z = _principal_pair(features, "umap_init")
    return (z * (10.0 / np.abs(z).max())).astype(np.float32)


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


# ---- UMAP ----------------------------------------------------------------------------------------------------------------------
UMAP_MIN_K, UMAP_MAX_K, UMAP_MAX_RATE = 2, 64, 16   # the limits of k_umap.hip (n and dim as above)


def check_umap_limits(n: int, dim: int, n_neighbors: int) -> None:
    """Raise ValueError naming the limit that (n, dim, n_neighbors) breaks: the library's own limits, checked before any buffer exists."""
    if not MIN_N <= n <= MAX_N:
        raise ValueError(f"DeviceUMAP: n = {n} outside [{MIN_N}, {MAX_N}]")
    if not 1 <= dim <= MAX_DIM:
        raise ValueError(f"DeviceUMAP: dim = {dim} outside [1, {MAX_DIM}]")
    if not (UMAP_MIN_K <= n_neighbors <= UMAP_MAX_K and n_neighbors < n):
        raise ValueError(f"DeviceUMAP: n_neighbors = {n_neighbors} outside [{UMAP_MIN_K}, min({UMAP_MAX_K}, n - 1 = {n - 1})]")


def find_ab_params(spread: float = 1.0, min_dist: float = 0.1) -> Tuple[float, float]:
    """(a, b) of umap-learn's find_ab_params: the least-squares fit of 1 / (1 + a x^(2 b)) to the target 1 for x < min_dist, else
    e^(-(x - min_dist) / spread), on linspace(0, 3 spread, 300).  Levenberg-Marquardt from (1, 1) in float64 numpy, run to a step below
    1e-13 of the parameters: the minimum scipy.optimize.curve_fit stops near (1.576943460, 0.895060878 for the defaults)."""
    xv = np.linspace(0.0, 3.0 * spread, 300)
    yv = np.where(xv < min_dist, 1.0, np.exp(-(xv - min_dist) / spread))
    lx = np.log(np.where(xv > 0, xv, 1.0))   # x = 0: x^(2 b) log x = 0

    def model(p):
        x2b = np.where(xv > 0, np.exp(2.0 * p[1] * lx), 0.0)
        f = 1.0 / (1.0 + p[0] * x2b)
        return f, np.stack([-f * f * x2b, -f * f * p[0] * x2b * 2.0 * lx], 1)

    p, lam = np.array([1.0, 1.0]), 1e-3
    f, J = model(p)
    cost = float(((f - yv) ** 2).sum())
    for _ in range(500):
        H, g = J.T @ J, J.T @ (f - yv)
        step = np.linalg.solve(H + lam * np.diag(np.diag(H)), -g)
        q = p + step
        if q[0] > 0 and q[1] > 0:
            fq, Jq = model(q)
            cq = float(((fq - yv) ** 2).sum())
        else:
            cq = np.inf
        if cq <= cost:
            done = np.abs(step).max() <= 1e-13 * np.abs(p).max()
            p, f, J, cost, lam = q, fq, Jq, cq, max(lam * 0.1, 1e-12)
            if done:
                break
        else:
            lam *= 10.0
            if lam > 1e12:
                break
    return float(p[0]), float(p[1])


def fuzzy_graph(knn_idx: torch.Tensor, memb: torch.Tensor, n_epochs: int) -> Dict:
    """The fuzzy union of the directed memberships as the CSR graph of ``mae_umap_epoch``, with torch ops on the device.
    knn_idx (n, k) int32 and memb (n, k) fp32 from ``mae_umap_fuzzy_knn``.  w_ij = (m_ij + m_ji) - (m_ij * m_ji), an absent direction 0,
    each operation rounded once in fp32 (W is symmetric bit for bit); edges with w < max(w) / n_epochs are dropped; eps = max(w) / w.
    -> dict(row_ptr (n + 1) int32, col (E) int32, eps (E), w (E) fp32, edges = E): both directions of every surviving edge, columns
    ascending within a row.  One host read (the edge count)."""
    n, k = memb.shape
    dev = memb.device
    rows = torch.arange(n, device=dev, dtype=torch.int64).repeat_interleave(k)
    cols = knn_idx.reshape(-1).to(torch.int64)
    fwd, order = torch.sort(rows * n + cols)         # a row's k neighbours are distinct: the keys are unique
    m = memb.reshape(-1).to(torch.float32)[order]
    keys = torch.unique(torch.cat([fwd, cols * n + rows]))   # ascending: row-major, columns ascending

    def lookup(q):
        pos = torch.searchsorted(fwd, q).clamp_(max=fwd.numel() - 1)
        return torch.where(fwd[pos] == q, m[pos], torch.zeros((), dtype=torch.float32, device=dev))

    ki, kj = torch.div(keys, n, rounding_mode="floor"), keys % n
    a, b = lookup(keys), lookup(kj * n + ki)
    w = (a + b) - (a * b)
    wmax = w.max()
    # a float64 quotient of fp32 values rounded to fp32 is the correctly rounded fp32 quotient (53 >= 2 * 24 + 2), whatever the device's
    # fp32 division does
    keep = (w >= (wmax.double() / float(n_epochs)).float()) & (w > 0)
    ki, kj, w = ki[keep], kj[keep], w[keep]          # the host read: the edge count
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(torch.bincount(ki, minlength=n), 0)
    return dict(row_ptr=row_ptr.to(torch.int32), col=kj.to(torch.int32).contiguous(), eps=(wmax.double() / w.double()).float().contiguous(),
                w=w.contiguous(), edges=int(w.numel()))


class DeviceUMAP:
    def __init__(self, n_neighbors: int = 15, min_dist: float = 0.1, spread: float = 1.0, n_epochs: Optional[int] = None, negative_sample_rate: int = 5,
                 learning_rate: float = 1.0, repulsion_strength: float = 1.0, seed: int = 73):
        if not UMAP_MIN_K <= int(n_neighbors) <= UMAP_MAX_K:
            raise ValueError(f"DeviceUMAP: n_neighbors = {n_neighbors} outside [{UMAP_MIN_K}, {UMAP_MAX_K}]")
        if not 1 <= int(negative_sample_rate) <= UMAP_MAX_RATE:
            raise ValueError(f"DeviceUMAP: negative_sample_rate = {negative_sample_rate} outside [1, {UMAP_MAX_RATE}]")
        if n_epochs is not None and not 1 <= int(n_epochs) < 2 ** 24:
            raise ValueError(f"DeviceUMAP: n_epochs = {n_epochs} outside [1, 2^24)")
        if not (spread > 0 and 0 <= min_dist <= spread):
            raise ValueError(f"DeviceUMAP: need spread > 0 and 0 <= min_dist <= spread, got min_dist = {min_dist}, spread = {spread}")
        if not (learning_rate > 0 and repulsion_strength >= 0):
            raise ValueError("DeviceUMAP: learning_rate must be > 0 and repulsion_strength >= 0")
        self.n_neighbors, self.min_dist, self.spread, self.n_epochs = int(n_neighbors), float(min_dist), float(spread), n_epochs and int(n_epochs)
        self.negative_sample_rate, self.learning_rate, self.repulsion_strength = int(negative_sample_rate), float(learning_rate), float(repulsion_strength)
        self.seed = int(seed) & 0xFFFFFFFF
        self.a, self.b = find_ab_params(self.spread, self.min_dist)
        self.n = 0
        self.epoch = 0

    # ---- state ------------------------------------------------------------------------------------------------------------
    def prepare(self, features: torch.Tensor, init, outputs: bool = False) -> "DeviceUMAP":
        """Build the graph of features (n, dim) on the device and set y = init (n, 2), next = eps, epoch = 0.
        outputs: also keep knn_idx, knn_dist, memb, rho and sigma (the tests read them)."""
        if features.dim() != 2:
            raise ValueError(f"DeviceUMAP: features must be (n, dim), got {tuple(features.shape)}")
        n, dim = features.shape
        check_umap_limits(n, dim, self.n_neighbors)
        if not features.is_cuda:
            raise RuntimeError("DeviceUMAP works on device tensors only (no CPU fallback); move the features to cuda")
        dev, k = features.device, self.n_neighbors
        x = features.detach().to(torch.float32).contiguous()
        y = torch.as_tensor(init, dtype=torch.float32).to(dev).contiguous().clone()
        if tuple(y.shape) != (n, 2):
            raise ValueError(f"DeviceUMAP: init must be ({n}, 2), got {tuple(y.shape)}")
        knn_idx = torch.empty((n, k), dtype=torch.int32, device=dev)
        knn_dist, memb = (torch.empty((n, k), dtype=torch.float32, device=dev) for _ in range(2))
        rho, sigma = (torch.empty(n, dtype=torch.float32, device=dev) for _ in range(2))
        scratch = torch.empty(lib.mae_umap_scratch_bytes(n, dim, k), dtype=torch.uint8, device=dev)
        check(lib.mae_umap_fuzzy_knn(_ptr(x), n, dim, k, _ptr(knn_idx), _ptr(knn_dist), _ptr(memb), _ptr(rho), _ptr(sigma), _ptr(scratch), scratch.numel(),
                                     _stream(dev)))
        self.n, self.device = n, dev
        self.epochs = self.n_epochs or (500 if n <= 10000 else 200)
        self.graph = fuzzy_graph(knn_idx, memb, self.epochs)
        del scratch
        self.knn_idx, self.knn_dist, self.memb, self.rho, self.sigma = (knn_idx, knn_dist, memb, rho, sigma) if outputs else (None,) * 5
        self.next = self.graph["eps"].clone()
        self.y, self._spare = y, torch.empty_like(y)
        self.epoch = 0
        return self

    def alpha(self, t: int) -> float:
        """The step of epoch t, rounded to fp32 on the host."""
        return float(np.float32(self.learning_rate * (1.0 - t / self.epochs)))

    def step(self, k: int = 1) -> "DeviceUMAP":
        """Advance k epochs; y, next and epoch stay readable.  No host synchronisation."""
        if self.n == 0:
            raise RuntimeError("DeviceUMAP.step before prepare")
        if self.epoch + int(k) > self.epochs:
            raise ValueError(f"DeviceUMAP.step: {k} epochs from epoch {self.epoch} pass n_epochs = {self.epochs}")
        g, s = self.graph, _stream(self.device)
        for _ in range(int(k)):
            check(lib.mae_umap_epoch(_ptr(self.y), _ptr(self._spare), _ptr(g["row_ptr"]), _ptr(g["col"]), _ptr(g["eps"]), _ptr(self.next), self.n,
                                     self.a, self.b, self.repulsion_strength, self.alpha(self.epoch), self.epoch, self.negative_sample_rate, self.seed, s))
            self.y, self._spare = self._spare, self.y
            self.epoch += 1
        return self

    def fit(self, features: torch.Tensor, init: Optional[object] = None) -> Tuple[torch.Tensor, Dict]:
        """-> (Z (n, 2) fp32 on the device, info).  init None = umap_init(features)."""
        init = umap_init(features) if init is None else init
        self.prepare(features, init)
        self.step(self.epochs)
        info = dict(n=self.n, epochs=self.epoch, n_neighbors=self.n_neighbors, min_dist=self.min_dist, a=self.a, b=self.b, edges=self.graph["edges"],
                    seed=self.seed)
        return self.y, info
