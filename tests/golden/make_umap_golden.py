"""Writes tests/golden/umap_blobs.json: the spread of the float64 UMAP reference (tests/umap_ref.py) on the blob data.  CPU only.

    python -m tests.golden.make_umap_golden

Nine reference fits (500 synchronous epochs from umap_init, k = 15), one per seed of the negative samples, and their trustworthiness at
15 neighbours and leave-one-out 1-NN label accuracy in the plane.  The device's limit is min - (max - min) of the nine trustworthiness
values, and the lowest of the nine accuracies: taken from the reference, never from the code under test.

One more run is recorded, not used as a limit: an in-order sequential restatement of umap-learn's optimize_layout_euclidean on the same
graph (in-place updates edge by edge, move_other, the running quotient of negative samples, numpy's generator for the negatives).  It
takes minutes in pure Python, which is why it is recorded here and not run in a test; it shows where the synchronous rule stands against
the rule it replaces.
"""
import json
from pathlib import Path

import numpy as np

from ssrl_vit_mae_jepa_amd.embedding import find_ab_params, umap_init
from tests import umap_ref as R

OUT = Path(__file__).resolve().parent / "umap_blobs.json"
SEEDS = tuple(range(73, 82))
K, EPOCHS, RATE = 15, 500, 5


def sequential(y0, g, a, b, n_epochs, rate=RATE, gamma=1.0, seed=1):
    """umap-learn's loop, one edge at a time in the order of the (symmetric) edge list."""
    y = np.asarray(y0, dtype=np.float64).copy()
    n = len(y)
    rows, cols = g["rows"], g["col"]
    eps = g["eps"].astype(np.float64)
    nxt, eps_neg = eps.copy(), eps / rate
    nxt_neg = eps_neg.copy()
    rng = np.random.default_rng(seed)
    for t in range(n_epochs):
        alpha = 1.0 - t / n_epochs
        for e in np.nonzero(nxt <= t)[0]:
            i, j = rows[e], cols[e]
            diff = y[i] - y[j]
            d2 = float(diff @ diff)
            if d2 > 0:
                step = alpha * np.clip(-2.0 * a * b * d2 ** (b - 1.0) / (a * d2 ** b + 1.0) * diff, -4.0, 4.0)
                y[i] += step
                y[j] -= step
            nxt[e] += eps[e]
            count = int((t - nxt_neg[e]) / eps_neg[e])
            for k in rng.integers(0, n, size=count):
                diff = y[i] - y[k]
                d2 = float(diff @ diff)
                if d2 > 0 and k != i:
                    y[i] += alpha * np.clip(2.0 * gamma * b / ((0.001 + d2) * (a * d2 ** b + 1.0)) * diff, -4.0, 4.0)
            nxt_neg[e] += count * eps_neg[e]
    return y


def main():
    x, labels = R.blobs()
    a, b = (float(np.float32(v)) for v in find_ab_params())   # the fp32 values the kernel is given
    g = R.graph_of(x, K, EPOCHS)
    y0 = umap_init(x)
    trust, acc = [], []
    for seed in SEEDS:
        Z = R.fit(x, y0, a, b, k=K, n_epochs=EPOCHS, rate=RATE, seed=seed, graph=g)["Z"]
        assert np.isfinite(Z).all()
        trust.append(R.trustworthiness(x, Z, 15))
        acc.append(R.loo_1nn_accuracy(Z, labels))
        print(f"seed {seed}: trustworthiness {trust[-1]:.6f}, leave-one-out 1-NN accuracy {acc[-1]:.4f}, max |y| {np.abs(Z).max():.2f}", flush=True)
    Zs = sequential(y0, g, a, b, EPOCHS)
    seq = dict(trustworthiness=R.trustworthiness(x, Zs, 15), accuracy=R.loo_1nn_accuracy(Zs, labels))
    print("sequential:", seq)
    OUT.write_text(json.dumps(dict(data="tsne_ref.blobs()", n_neighbors=K, n_epochs=EPOCHS, negative_sample_rate=RATE, seeds=list(SEEDS), a=a, b=b,
                                   edges=int(len(g["col"])), trustworthiness=trust, accuracy=acc, limit=min(trust) - (max(trust) - min(trust)),
                                   accuracy_limit=min(acc), sequential=seq), indent=1) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
