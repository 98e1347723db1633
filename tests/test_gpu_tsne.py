"""embedding.DeviceTSNE end to end on the MI355X, on the blob data of tests/tsne_ref.py (600 points, 6 clusters, dim 32):

  one step     at iterations 0, 1, 249, 250 and 999 the device's state is handed to the float64 reference for one step, and the device's
               next (y, update, gains) must lie inside the one-step bound (the gradient bound carried through lr * gains); gains exactly,
               except where |grad| is below its own bound and the sign of update * grad may flip
  quality      after 1000 iterations from pca_init: leave-one-out 1-NN label accuracy 1.0 in the plane, and a final KL no worse than
               max + (max - min) of the float64 reference's nine runs (tests/golden/tsne_blobs_kl.json)
  reproducible two fits, the same bits in Z and in the KL trace
  CLI          --method tsne_gpu writes the figures, the .npz and the .json
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import tsne_ref as T

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SNAPSHOTS = (0, 1, 249, 250, 999)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def blob_run(dev):
    """One prepare + 1000 iterations, with the state before and after the snapshot iterations; shared, never modified."""
    from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE, pca_init
    x, labels = T.blobs()
    tsne = DeviceTSNE(perplexity=30.0)
    tsne.prepare(torch.from_numpy(x).to(dev), pca_init(x))
    P = np_(tsne.P)[:, :600].astype(np.float64)
    snaps = {}
    for it in SNAPSHOTS:
        tsne.step(it - tsne.iteration)
        before = tuple(np_(v).copy() for v in (tsne.y, tsne.update, tsne.gains))
        tsne.step(1)
        snaps[it] = (before, tuple(np_(v).copy() for v in (tsne.y, tsne.update, tsne.gains, tsne.grad)))
    assert tsne.iteration == 1000
    kl = float(tsne.kl_divergence().item())
    return dict(P=P, snaps=snaps, Z=np_(tsne.y), labels=labels, kl=kl, x=x)


@pytest.mark.parametrize("it", SNAPSHOTS)
def test_one_step_against_float64(blob_run, it):
    (y, upd, gains), (y1, u1, g1, grad) = blob_run["snaps"][it]
    ref = T.one_step(blob_run["P"], y, upd, gains, it)
    rg = np.abs(grad.astype(np.float64) - ref["grad"]) / ref["grad_bound"]
    ru = np.abs(u1.astype(np.float64) - ref["update"]) / ref["update_bound"]
    ry = np.abs(y1.astype(np.float64) - ref["y"]) / ref["y_bound"]
    exact = ref["exact_gains"]
    print(f"iteration {it}: grad {rg.max():.3g} update {ru.max():.3g} y {ry.max():.3g} of their bounds; {int((~exact).sum())} coordinates whose sign may flip")
    assert rg.max() <= 1.0 and ru.max() <= 1.0 and ry.max() <= 1.0
    assert (g1[exact] == ref["gains32"][exact]).all()   # the fp32 operation on the branch the float64 gradient takes
    assert exact.mean() > 0.99


def test_quality_band(blob_run):
    golden = json.loads((ROOT / "tests" / "golden" / "tsne_blobs_kl.json").read_text())
    limit = max(golden["kl"]) + (max(golden["kl"]) - min(golden["kl"]))
    acc = T.loo_1nn_accuracy(blob_run["Z"], blob_run["labels"])
    print(f"device KL {blob_run['kl']:.6f}; float64 runs {min(golden['kl']):.6f} .. {max(golden['kl']):.6f}, limit {limit:.6f}; accuracy {acc}")
    assert np.isfinite(blob_run["Z"]).all()
    assert acc == 1.0
    assert blob_run["kl"] <= limit
    ref = T.gradient(blob_run["P"], blob_run["Z"], 1.0)   # the device's KL is the KL of its own embedding
    assert abs(blob_run["kl"] - ref["kl"]) <= T.kl_bound(ref, 600)


def test_fit_is_reproducible(dev, blob_run):
    from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE
    x = torch.from_numpy(blob_run["x"]).to(dev)
    Za, ia = DeviceTSNE(perplexity=30.0).fit(x)
    Zb, ib = DeviceTSNE(perplexity=30.0).fit(x)
    assert torch.equal(Za, Zb) and ia == ib
    assert ia["iterations"] == 1000 and ia["n"] == 600 and ia["learning_rate"] == 50.0
    assert [it for it, _ in ia["kl_trace"]] == list(range(50, 1001, 50))
    assert (np_(Za) == blob_run["Z"]).all()                  # prepare + step and fit walk the same path
    assert ia["kl_divergence"] == blob_run["kl"]
    early, late = ia["kl_trace"][4][1], ia["kl_trace"][-1][1]
    assert np.isfinite([v for _, v in ia["kl_trace"]]).all() and late < early


def test_cli_writes_figures_npz_and_json(dev, tmp_path):
    from scripts.evaluation import visualize_representation as V
    save_dir, stem = V.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--encoder_ckpt", "random", "--method", "tsne_gpu", "--pool", "mean",
                             "--normalize", "channel", "--batch_size", "64", "--synthetic_images", "200", "--max_samples", "200",
                             "--output_dir", str(tmp_path), "--save_features"])
    assert "tsne_gpu" in stem
    assert (save_dir / f"{stem}.png").exists() and list(save_dir.glob(f"{stem}_class*.png"))
    z = np.load(save_dir / f"{stem}.npz")
    assert z["projection"].shape == (200, 2) and np.isfinite(z["projection"]).all()
    info = json.loads((save_dir / f"{stem}.json").read_text())
    assert info["n"] == 200 and info["iterations"] == 1000 and len(info["kl_trace"]) == 20 and np.isfinite(info["kl_divergence"])
