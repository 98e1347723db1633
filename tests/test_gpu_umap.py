"""embedding.DeviceUMAP end to end on the MI355X, on the blob data of tests/tsne_ref.py (600 points, 6 clusters, dim 32):

  graph        fuzzy_graph on the device's own lists equals the fp32 restatement's CSR: the same structure, w and eps bit for bit
  one step     at epochs 1, 2, 250 and 499 the device's positions and schedule are handed to the float64 reference for one epoch, and the
               device's next positions must lie inside the counted bound; next and the active set bit for bit
  quality      after 500 epochs from umap_init: trustworthiness at 15 neighbours no worse than min - (max - min) of the float64
               reference's nine runs, leave-one-out 1-NN accuracy no worse than their lowest (tests/golden/umap_blobs.json)
  reproducible two fits, the same bits in Z
  CLI          --method umap_gpu writes the figures, the .npz and the .json; --max_samples above 16384 is refused by name
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import umap_ref as R

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
SNAPSHOTS = (1, 2, 250, 499)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def blob_run(dev):
    """One prepare + 500 epochs, with the state before and after the snapshot epochs; shared, never modified."""
    from ssrl_vit_mae_jepa_amd.embedding import DeviceUMAP, umap_init
    x, labels = R.blobs()
    um = DeviceUMAP()
    um.prepare(torch.from_numpy(x).to(dev), umap_init(x), outputs=True)
    lists = {k: np_(getattr(um, k)).copy() for k in ("knn_idx", "knn_dist", "memb", "rho", "sigma")}
    graph = {k: np_(v).copy() for k, v in um.graph.items() if k != "edges"}
    snaps = {}
    for t in SNAPSHOTS:
        um.step(t - um.epoch)
        before = (np_(um.y).copy(), np_(um.next).copy())
        um.step(1)
        snaps[t] = (before, (np_(um.y).copy(), np_(um.next).copy()))
    assert um.epoch == um.epochs == 500
    return dict(x=x, labels=labels, lists=lists, graph=graph, edges=um.graph["edges"], snaps=snaps, Z=np_(um.y).copy(), a=um.a, b=um.b, seed=um.seed)


def test_fuzzy_graph_equals_the_fp32_restatement(blob_run):
    g, lists = blob_run["graph"], blob_run["lists"]
    ref = R.fuzzy_union(lists["knn_idx"], lists["memb"], 500)
    assert g["row_ptr"].dtype == np.int32 and g["col"].dtype == np.int32 and blob_run["edges"] == len(g["col"]) == len(ref["col"])
    assert (g["row_ptr"] == ref["row_ptr"]).all() and (g["col"] == ref["col"]).all()
    assert (g["w"].view(np.uint32) == ref["w"].view(np.uint32)).all() and (g["eps"].view(np.uint32) == ref["eps"].view(np.uint32)).all()
    host = R.graph_of(blob_run["x"], 15, 500)
    print(f"{len(g['col'])} directed edges on the device, {len(host['col'])} in the float64 reference; eps {g['eps'].min()} .. {g['eps'].max()}")
    assert abs(len(g["col"]) - len(host["col"])) <= 0.01 * len(host["col"])


@pytest.mark.parametrize("t", SNAPSHOTS)
def test_one_epoch_against_float64(blob_run, t):
    (y, nxt), (y1, nxt1) = blob_run["snaps"][t]
    g = blob_run["graph"]
    a, b = (float(np.float32(v)) for v in (blob_run["a"], blob_run["b"]))
    ref = R.epoch(y, g["row_ptr"], g["col"], g["eps"], nxt, a, b, 1.0, R.alpha_of(t, 500), t, 5, blob_run["seed"])
    assert (nxt1.view(np.uint32) == ref["next"].view(np.uint32)).all()
    ratio = np.abs(y1.astype(np.float64) - ref["y"]) / ref["bound"]
    print(f"epoch {t}: {int(ref['active'].sum())} of {len(nxt)} edges fire; y error / bound {ratio.max():.3g}; max |y| {np.abs(y1).max():.2f}")
    assert ref["active"].any() and ratio.max() <= 1.0


def test_quality_band(blob_run):
    golden = json.loads((ROOT / "tests" / "golden" / "umap_blobs.json").read_text())
    lo, hi = min(golden["trustworthiness"]), max(golden["trustworthiness"])
    limit, acc_limit = lo - (hi - lo), min(golden["accuracy"])
    Z = blob_run["Z"]
    assert np.isfinite(Z).all()
    trust, acc = R.trustworthiness(blob_run["x"], Z, 15), R.loo_1nn_accuracy(Z, blob_run["labels"])
    print(f"device trustworthiness {trust:.6f}; float64 runs {lo:.6f} .. {hi:.6f}, limit {limit:.6f}; accuracy {acc} (limit {acc_limit}); max |y| {np.abs(Z).max():.2f}")
    assert trust >= limit
    assert acc >= acc_limit


def test_fit_is_reproducible_and_info_is_complete(dev, blob_run):
    from ssrl_vit_mae_jepa_amd.embedding import DeviceUMAP
    x = torch.from_numpy(blob_run["x"]).to(dev)
    Za, ia = DeviceUMAP().fit(x)
    Zb, ib = DeviceUMAP().fit(x)
    assert torch.equal(Za, Zb) and ia == ib
    assert (np_(Za) == blob_run["Z"]).all()                  # prepare + step and fit walk the same path
    assert set(ia) == {"n", "epochs", "n_neighbors", "min_dist", "a", "b", "edges", "seed"}
    assert ia["n"] == 600 and ia["epochs"] == 500 and ia["n_neighbors"] == 15 and ia["min_dist"] == 0.1 and ia["seed"] == 73
    assert ia["edges"] == blob_run["edges"] and abs(ia["a"] - 1.576943460) < 1e-5 and abs(ia["b"] - 0.895060878) < 1e-5
    json.dumps(ia)
    Zc, _ = DeviceUMAP(seed=74).fit(x)
    assert not torch.equal(Za, Zc)


def test_cli_writes_figures_npz_and_json(dev, tmp_path):
    from scripts.evaluation import visualize_representation as V
    save_dir, stem = V.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--encoder_ckpt", "random", "--method", "umap_gpu", "--pool", "mean",
                             "--normalize", "channel", "--batch_size", "64", "--synthetic_images", "200", "--max_samples", "200",
                             "--output_dir", str(tmp_path), "--save_features"])
    assert "umap_gpu" in stem
    assert (save_dir / f"{stem}.png").exists() and list(save_dir.glob(f"{stem}_class*.png"))
    z = np.load(save_dir / f"{stem}.npz")
    assert z["projection"].shape == (200, 2) and np.isfinite(z["projection"]).all()
    info = json.loads((save_dir / f"{stem}.json").read_text())
    assert info["n"] == 200 and info["epochs"] == 500 and info["n_neighbors"] == 15 and info["edges"] > 0


def test_cli_refuses_more_samples_than_the_device_admits():
    from scripts.evaluation import visualize_representation as V
    with pytest.raises(SystemExit, match="--method umap_gpu embeds at most 16384 samples, --max_samples is 20000"):
        V.main(["--encoder_ckpt", "random", "--method", "umap_gpu", "--synthetic_images", "200", "--max_samples", "20000"])
