"""What the device t-SNE costs, printed as one JSON document: n in {2000, 8000, 16384}, dim 384, clustered synthetic features.

In one process and with the same device events, per n:
  * `mae_tsne_gradient` alone against the n^2 * 4 bytes of P it streams, beside the yardstick of tools/hbm_stream_reference.py measured
    here on a buffer of the same size: torch's device copy (read + write) and sum (read);
  * `mae_tsne_step` (gradient + descent step: one iteration), `mae_tsne_affinities`, and a whole `DeviceTSNE.fit` from a given
    initialisation (1000 iterations, wall clock around one synchronisation);
  * `sklearn.manifold.TSNE` as `visualize_representation.py --method tsne` runs it (Barnes-Hut, on the host's CPUs), at the sizes of
    `--sklearn` (default 2000 and 8000), once each.
Every device figure is the median of `--repeats` windows; the windows of the cases alternate, so a drift of the clocks falls on all of
them alike.  No threshold: the table says where the gradient sits against the stream.

    python tools/tsne_bench.py --out profiles/r30_tsne_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

from classifier_bench import timed  # noqa: E402
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE, pca_init  # noqa: E402

SIZES = (2000, 8000, 16384)
DIM = 384


def clustered(n: int, dim: int = DIM, clusters: int = 10, seed: int = 0) -> np.ndarray:
    r = np.random.default_rng([n, seed])
    return (4.0 * r.standard_normal((clusters, dim))[r.integers(0, clusters, n)] + r.standard_normal((n, dim))).astype(np.float32)


def bench(n, steps, warmup, repeats, dev) -> dict:
    lib, stream = _lib.lib, torch.cuda.current_stream(dev).cuda_stream
    x_host = clustered(n)
    x = torch.from_numpy(x_host).to(dev)
    init = pca_init(x_host)
    tsne = DeviceTSNE(perplexity=30.0)
    tsne.prepare(x, init)
    tsne.step(300)   # past the exaggeration: the embedding has spread, as in most of a fit
    P, y, grad, scratch = tsne.P, tsne.y, torch.empty_like(tsne.y), tsne.scratch
    y2, u2, g2 = tsne.y.clone(), tsne.update.clone(), tsne.gains.clone()
    P2 = torch.empty_like(P)
    kl = torch.empty(1, device=dev)
    a, b = torch.empty(n * n, device=dev), torch.empty(n * n, device=dev)
    a.uniform_()

    def gradient():
        _lib.check(lib.mae_tsne_gradient(P.data_ptr(), y.data_ptr(), n, 1.0, grad.data_ptr(), None, scratch.data_ptr(), scratch.numel(), stream))

    def gradient_kl():
        _lib.check(lib.mae_tsne_gradient(P.data_ptr(), y.data_ptr(), n, 1.0, grad.data_ptr(), kl.data_ptr(), scratch.data_ptr(), scratch.numel(), stream))

    def step():
        _lib.check(lib.mae_tsne_step(P.data_ptr(), y2.data_ptr(), u2.data_ptr(), g2.data_ptr(), n, 1.0, 0.8, 50.0, 0.01, grad.data_ptr(), None,
                                     scratch.data_ptr(), scratch.numel(), stream))

    def affinities():
        _lib.check(lib.mae_tsne_affinities(x.data_ptr(), n, DIM, 30.0, P2.data_ptr(), None, None, None, stream))

    cases = {"gradient": (gradient, steps), "gradient_with_kl": (gradient_kl, steps), "step": (step, steps), "affinities": (affinities, 2),
             "torch_copy": (lambda: b.copy_(a), steps), "torch_sum": (lambda: a.sum(), steps)}
    runs = {k: [] for k in cases}
    for _ in range(repeats):   # alternated windows
        for k, (fn, cnt) in cases.items():
            runs[k].append(timed(fn, cnt, min(warmup, cnt)))
    ms = {k: statistics.median(v) for k, v in runs.items()}
    del a, b, P2
    fits = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        DeviceTSNE(perplexity=30.0).fit(x, init)
        fits.append(time.perf_counter() - t0)   # fit ends in the one read of the KL trace
    stream_bytes = 4.0 * n * n
    copy_tbs, sum_tbs, grad_tbs = 2 * stream_bytes / ms["torch_copy"] / 1e9, stream_bytes / ms["torch_sum"] / 1e9, stream_bytes / ms["gradient"] / 1e9
    return {"n": n, "dim": DIM, "ms": ms, "ms_all": runs, "p_bytes": stream_bytes, "gradient_tb_per_s": grad_tbs, "torch_copy_tb_per_s": copy_tbs,
            "torch_sum_tb_per_s": sum_tbs, "gradient_over_copy_rate": grad_tbs / copy_tbs, "pairs_per_ns": n * n / ms["gradient"] / 1e6,
            "fit_1000_iterations_s": statistics.median(fits), "fit_s_all": fits}


def sklearn_tsne(n: int) -> dict:
    from sklearn.manifold import TSNE
    x = clustered(n)
    t0 = time.perf_counter()
    est = TSNE(n_components=2, perplexity=30.0, learning_rate="auto", random_state=73)
    est.fit_transform(x)
    return {"n": n, "seconds": time.perf_counter() - t0, "iterations": int(est.n_iter_), "kl_divergence": float(est.kl_divergence_), "method": "barnes_hut"}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=40, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--sklearn", default="2000,8000", help="sizes at which sklearn's TSNE is timed on the host ('' = none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/tsne_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "cases": [], "sklearn": [], "notes": []}
    for n in (int(v) for v in args.sizes.split(",") if v):
        r = bench(n, args.steps, args.warmup, args.repeats, dev)
        out["cases"].append(r)
        out["notes"].append(f"n = {n}: gradient {r['ms']['gradient'] * 1e3:.1f} us = {r['gradient_tb_per_s']:.2f} TB/s of P (torch copy {r['torch_copy_tb_per_s']:.2f}, "
                            f"sum {r['torch_sum_tb_per_s']:.2f} TB/s on the same bytes), {r['pairs_per_ns']:.1f} pairs / ns; step {r['ms']['step'] * 1e3:.1f} us; "
                            f"affinities {r['ms']['affinities']:.2f} ms; fit of 1000 iterations {r['fit_1000_iterations_s']:.3f} s")
        print(out["notes"][-1], flush=True)
        torch.cuda.empty_cache()
    for n in (int(v) for v in args.sklearn.split(",") if v):
        out["sklearn"].append(sklearn_tsne(n))
        print(out["sklearn"][-1], flush=True)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
