"""The host side of the device t-SNE (no GPU): schedule, pca_init, limit refusals, the CLI parser, and header, exports and binding
in step."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import tsne_ref as T

ROOT = Path(__file__).resolve().parents[1]
SYMBOLS = ("mae_tsne_affinities", "mae_tsne_gradient", "mae_tsne_update")


def test_schedule_values():
    from ssrl_vit_mae_jepa_amd.embedding import schedule
    assert schedule(0, 600)["learning_rate"] == 50.0                         # max(600 / 12 / 4, 50)
    assert schedule(0, 16384)["learning_rate"] == pytest.approx(16384 / 48.0)
    assert schedule(0, 600, learning_rate=200.0)["learning_rate"] == 200.0
    for it, mom, alpha in ((0, 0.5, 12.0), (249, 0.5, 12.0), (250, 0.8, 1.0), (999, 0.8, 1.0)):
        s = schedule(it, 600)
        assert (s["momentum"], s["alpha"]) == (mom, alpha)
        r = T.schedule(it, 600)
        assert (r["momentum"], r["alpha"], r["learning_rate"]) == (mom, alpha, s["learning_rate"])


def test_pca_init_scaling_and_directions():
    from ssrl_vit_mae_jepa_amd.embedding import pca_init
    x, _ = T.blobs()
    z = pca_init(x)
    assert z.shape == (600, 2) and z.dtype == np.float32
    assert np.std(z[:, 0].astype(np.float64)) == pytest.approx(1e-4, rel=1e-6)
    assert np.std(z[:, 0]) >= np.std(z[:, 1]) > 0
    assert abs(np.dot(z[:, 0].astype(np.float64), z[:, 1])) <= 1e-6 * np.linalg.norm(z[:, 0]) * np.linalg.norm(z[:, 1])   # uncorrelated
    # up to the sign of each component, sklearn's PCA and the wide branch (dim > n) agree
    from sklearn.decomposition import PCA
    sk = PCA(n_components=2, svd_solver="full").fit_transform(x.astype(np.float64))
    sk = sk / np.std(sk[:, 0]) * 1e-4
    np.testing.assert_allclose(np.abs(z), np.abs(sk), rtol=1e-3, atol=1e-9)
    wide = np.random.default_rng(0).standard_normal((20, 50))
    zw = pca_init(wide)
    skw = PCA(n_components=2, svd_solver="full").fit_transform(wide)
    np.testing.assert_allclose(np.abs(zw), np.abs(skw / np.std(skw[:, 0]) * 1e-4), rtol=1e-3, atol=1e-9)
    # a shift of the data and a flip of its sign change the map by at most a sign per component
    np.testing.assert_allclose(np.abs(pca_init(-x + 3.0)), np.abs(z), rtol=1e-3, atol=1e-9)


@pytest.mark.parametrize("n,dim,perp,word", [(7, 4, 2.0, "n = 7"), (16385, 4, 30.0, "n = 16385"), (100, 8193, 30.0, "dim = 8193"),
                                             (100, 4, 99.0, "perplexity"), (100, 4, 0.5, "perplexity")])
def test_limits_are_refused_by_name(n, dim, perp, word):
    from ssrl_vit_mae_jepa_amd.embedding import check_limits
    with pytest.raises(ValueError, match=word):
        check_limits(n, dim, perp)
    check_limits(8, 1, 1.0)
    check_limits(16384, 8192, 16382.0)


def test_prepare_refuses_before_touching_a_device():
    import torch
    from ssrl_vit_mae_jepa_amd.embedding import DeviceTSNE
    with pytest.raises(ValueError, match="n = 7"):
        DeviceTSNE(perplexity=2.0).prepare(torch.zeros(7, 4), np.zeros((7, 2)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        DeviceTSNE(perplexity=2.0).prepare(torch.zeros(9, 4), np.zeros((9, 2)))


def test_library_limits_without_buffers():
    from ssrl_vit_mae_jepa_amd._lib import lib
    assert lib.mae_tsne_pitch(7) == -1 and lib.mae_tsne_pitch(16385) == -1
    assert [lib.mae_tsne_pitch(n) for n in (8, 63, 65, 1030, 16384)] == [8, 64, 68, 1032, 16384]
    assert lib.mae_tsne_scratch_bytes(7, 4) == -1 and lib.mae_tsne_scratch_bytes(100, 0) == -1 and lib.mae_tsne_scratch_bytes(100, 8193) == -1
    assert lib.mae_tsne_scratch_bytes(1030, 384) == 6 * 1032 * 4
    for n, perp, word in ((7, 2.0, b"n = 7"), (16385, 30.0, b"n = 16385"), (100, 99.0, b"perplexity")):
        assert lib.mae_tsne_affinities(None, n, 4, perp, None, None, None, None, None) != 0   # refused before any pointer is touched
        assert word in lib.mae_last_error()


def test_cli_parser_and_sample_limit():
    from scripts.evaluation import visualize_representation as V
    args = V.parse_args(["--encoder_ckpt", "random", "--method", "tsne_gpu"])
    assert args.method == "tsne_gpu" and args.max_samples == 2000
    assert V.parse_args(["--encoder_ckpt", "random"]).method == "umap"       # the default stays
    with pytest.raises(SystemExit):
        V.parse_args(["--encoder_ckpt", "random", "--method", "tsne_cpu"])
    with pytest.raises(SystemExit, match="16384"):                            # before the config, the encoder or any image is read
        V.main(["--config", "does/not/exist.yaml", "--encoder_ckpt", "random", "--method", "tsne_gpu", "--max_samples", "16385"])


def test_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    header = (ROOT / "include" / "mae_hip.h").read_text()
    for name in SYMBOLS + ("mae_tsne_step", "mae_tsne_pitch", "mae_tsne_scratch_bytes"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in _lib.SIGNATURES and hasattr(_lib.lib, name)
    assert _lib.lib.mae_abi_version() == 4


def test_golden_kl_spread_is_recorded():
    import json
    g = json.loads((ROOT / "tests" / "golden" / "tsne_blobs_kl.json").read_text())
    assert len(g["kl"]) == 9 and g["limit"] == pytest.approx(max(g["kl"]) + (max(g["kl"]) - min(g["kl"])))
    assert g["accuracy"] == [1.0] * 9
