"""What the device UMAP costs, printed as one JSON document: n in {2000, 8000, 16384}, dim 384, clustered synthetic features.

In one process and with the same device events, per n:
  * `mae_umap_fuzzy_knn` (distances, selection, sigma search, memberships), `embedding.fuzzy_graph` (the torch assembly, wall clock around
    its one host read), and `mae_umap_epoch` as consecutive real epochs of a 500-epoch fit from epoch 100 on (the schedule advances as in
    a fit: a repeated epoch would soon fire nothing);
  * beside the epoch, its two yardsticks, measured here: the same kernel at t = 0, where no edge fires (the launch, the row walk and the
    read of `next`: what is left when no position is gathered), and torch's gather `y[idx]` of as many random rows of the same (n, 2)
    table as the epoch reads (fired edges x (rate + 1)), written to a buffer: the random reads alone, in one launch;
  * a whole `DeviceUMAP.fit` from a given initialisation (default epochs; wall clock around one synchronisation), beside
    `DeviceTSNE.fit` on the same features, and `sklearn.manifold.TSNE` (Barnes-Hut, on the host's CPUs) at the sizes of `--sklearn`.
Every device figure is the median of `--repeats` windows; the windows of the cases alternate, so a drift of the clocks falls on all of
them alike.  No threshold.

    python tools/umap_bench.py --out profiles/r32_umap_bench.json
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
from tsne_bench import DIM, SIZES, clustered, sklearn_tsne  # noqa: E402
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE, DeviceUMAP, fuzzy_graph, pca_init, umap_init  # noqa: E402

K = 15


def bench(n, steps, warmup, repeats, dev) -> dict:
    lib, stream = _lib.lib, torch.cuda.current_stream(dev).cuda_stream
    x_host = clustered(n)
    x = torch.from_numpy(x_host).to(dev)
    init = umap_init(x_host)
    um = DeviceUMAP(n_epochs=500)
    um.prepare(x, init, outputs=True)
    um.step(100)
    g, rate = um.graph, um.negative_sample_rate
    idx, dist, memb = (torch.empty_like(v) for v in (um.knn_idx, um.knn_dist, um.memb))
    rho, sigma = torch.empty_like(um.rho), torch.empty_like(um.sigma)
    nbytes = lib.mae_umap_scratch_bytes(n, DIM, K)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    idle_next, spare = g["eps"].clone(), torch.empty_like(um.y)
    fired = []

    def fuzzy_knn():
        _lib.check(lib.mae_umap_fuzzy_knn(x.data_ptr(), n, DIM, K, idx.data_ptr(), dist.data_ptr(), memb.data_ptr(), rho.data_ptr(), sigma.data_ptr(),
                                          scratch.data_ptr(), nbytes, stream))

    def epoch():
        um.step(1)

    def idle_epoch():   # t = 0: eps >= 1, nothing fires and next is not written
        _lib.check(lib.mae_umap_epoch(um.y.data_ptr(), spare.data_ptr(), g["row_ptr"].data_ptr(), g["col"].data_ptr(), g["eps"].data_ptr(),
                                      idle_next.data_ptr(), n, um.a, um.b, 1.0, 1.0, 0, rate, um.seed, stream))

    fired.append(int((um.next <= um.epoch).sum()))
    reads = max(1, fired[0] * (rate + 1))
    pick = torch.randint(0, n, (reads,), device=dev)
    gathered = torch.empty((reads, 2), dtype=torch.float32, device=dev)

    def gather():
        torch.index_select(um.y, 0, pick, out=gathered)

    cases = {"fuzzy_knn": (fuzzy_knn, 2), "epoch": (epoch, steps), "idle_epoch": (idle_epoch, steps), "torch_gather": (gather, steps)}
    runs = {k: [] for k in cases}
    for _ in range(repeats):   # alternated windows
        for k, (fn, cnt) in cases.items():
            runs[k].append(timed(fn, cnt, min(warmup, cnt)))
        fired.append(int((um.next <= um.epoch).sum()))
    ms = {k: statistics.median(v) for k, v in runs.items()}
    graphs = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fuzzy_graph(um.knn_idx, um.memb, 500)
        torch.cuda.synchronize()
        graphs.append((time.perf_counter() - t0) * 1e3)
    last_epoch = um.epoch
    del scratch
    fits, tsne_fits = [], []
    tsne_init = pca_init(x_host)
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        Z, info = DeviceUMAP().fit(x, init)
        Z.sum().item()
        fits.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        DeviceTSNE(perplexity=30.0).fit(x, tsne_init)   # ends in the one read of the KL trace
        tsne_fits.append(time.perf_counter() - t0)
    return {"n": n, "dim": DIM, "n_neighbors": K, "edges": g["edges"], "ms": ms, "ms_all": runs, "fuzzy_graph_ms": statistics.median(graphs), "fuzzy_graph_ms_all": graphs,
            "epochs_timed": [100, last_epoch], "fired_edges": fired, "reads_per_epoch": reads, "gather_bytes": 8 * reads,
            "epoch_over_idle": ms["epoch"] / ms["idle_epoch"], "epoch_over_gather": ms["epoch"] / ms["torch_gather"],
            "fit_epochs": info["epochs"], "fit_s": statistics.median(fits), "fit_s_all": fits, "tsne_fit_1000_iterations_s": statistics.median(tsne_fits),
            "tsne_fit_s_all": tsne_fits}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=40, help="calls per timed window")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", default=",".join(str(n) for n in SIZES))
    ap.add_argument("--sklearn", default="2000,8000", help="sizes at which sklearn's TSNE is timed on the host ('' = none)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.repeats * (args.steps + args.warmup) > 399:
        ap.error("repeats x (steps + warmup) epochs must fit between epoch 100 and 499")
    dev = torch.device("cuda", 0)
    out = {"tool": "tools/umap_bench.py", "argv": sys.argv[1:], "device": torch.cuda.get_device_name(0), "cases": [], "sklearn": [], "notes": []}
    for n in (int(v) for v in args.sizes.split(",") if v):
        r = bench(n, args.steps, args.warmup, args.repeats, dev)
        out["cases"].append(r)
        out["notes"].append(f"n = {n}: {r['edges']} directed edges; fuzzy_knn {r['ms']['fuzzy_knn']:.2f} ms; graph assembly {r['fuzzy_graph_ms']:.2f} ms; epoch "
                            f"{r['ms']['epoch'] * 1e3:.1f} us with {r['fired_edges'][0]} .. {r['fired_edges'][-1]} edges firing (idle epoch {r['ms']['idle_epoch'] * 1e3:.1f} us, "
                            f"torch gather of {r['reads_per_epoch']} rows {r['ms']['torch_gather'] * 1e3:.1f} us); fit of {r['fit_epochs']} epochs {r['fit_s']:.3f} s; "
                            f"t-SNE fit of 1000 iterations {r['tsne_fit_1000_iterations_s']:.3f} s")
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
