"""Writes tests/golden/tsne_blobs_kl.json: the spread of the float64 t-SNE reference (tests/tsne_ref.py) on the blob data.  CPU only.

    python -m tests.golden.make_tsne_golden

Run 0 starts from pca_init; runs 1..8 from pca_init times (1 + 1e-7 N(0, 1)) per coordinate, a perturbation below fp32 resolution.
After 1000 iterations the final KL divergences differ in the third digit: the descent is chaotic, and an fp32 run cannot be asked to
land closer to one float64 run than float64 runs land to each other.  The device's limit is max + (max - min) of the nine values.
"""
import json
from pathlib import Path

import numpy as np

from ssrl_vit_mae_jepa_amd.embedding import pca_init
from tests import tsne_ref as T

OUT = Path(__file__).resolve().parent / "tsne_blobs_kl.json"


def main():
    x, labels = T.blobs()
    P = T.affinities(x, 30.0)
    init = pca_init(x).astype(np.float64)
    r = np.random.default_rng(0)
    kls, accs = [], []
    for run in range(9):
        y0 = init if run == 0 else init * (1.0 + 1e-7 * r.standard_normal(init.shape))
        out = T.fit(x, y0, P=P)
        kls.append(out["kl"])
        accs.append(T.loo_1nn_accuracy(out["Z"], labels))
        print(f"run {run}: KL {kls[-1]:.6f}, leave-one-out 1-NN accuracy {accs[-1]:.4f}")
    OUT.write_text(json.dumps(dict(data="tsne_ref.blobs()", perplexity=30.0, max_iter=1000, kl=kls, accuracy=accs,
                                   limit=max(kls) + (max(kls) - min(kls))), indent=1) + "\n")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
