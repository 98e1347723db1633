"""Representation evaluation without a GPU: the C ABI names, workspace / scratch metadata, checkpoint layouts and encoder
loading on CPU state dicts, the host normalisation formulas and the k-NN CLI's argument checks."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"

NEW_SYMBOLS = ("mae_engine_features_workspace_bytes", "mae_engine_extract_features", "mae_knn_scratch_bytes", "mae_knn_topk", "mae_knn_vote")
TINY = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=2, num_heads=2))


def test_new_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for n in NEW_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert "MAE_POOL_MEAN_PATCHES = 2" in HEADER.read_text() and "MAE_FEAT_L2 = 1" in HEADER.read_text()
    assert (_lib.POOL_MEAN_PATCHES, _lib.FEAT_NONE, _lib.FEAT_L2) == (2, 0, 1) and _lib.ABI_VERSION == 4


def test_features_workspace_metadata_vits8():
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd.mae import Engine
    e = Engine(dict(image_size=96, patch_size=8, in_chans=3, embed_dim=384, depth=12, num_heads=6, decoder_embed_dim=512,
                    decoder_depth=8, decoder_num_heads=16), "bf16")
    h, B = e.handle, 2000
    no_cls = _lib.lib.mae_engine_features_workspace_bytes(h, B, 0)
    cls = _lib.lib.mae_engine_features_workspace_bytes(h, B, 1)
    clf = _lib.lib.mae_engine_classifier_workspace_bytes(h, B, 10)
    assert 0 < no_cls <= cls < clf
    for bad in ((0, 1), (-3, 0), (B, 2), (B, -1)):
        assert _lib.lib.mae_engine_features_workspace_bytes(h, *bad) == -1
    assert _lib.lib.mae_engine_features_workspace_bytes(None, B, 1) == -1


def test_knn_scratch_metadata():
    from ssrl_vit_mae_jepa_amd import _lib
    f = _lib.lib.mae_knn_scratch_bytes
    assert f(8000, 5000, 384, 200) >= 8000 * 200 * 8
    assert f(1, 1, 4, 1) > 0 and f(64, 100_000, 384, 20) > 0
    for bad in ((8000, 5000, 386, 20), (8000, 5000, 0, 20), (8000, 5000, 4100, 20), (8000, 5000, 384, 0), (8000, 5000, 384, 257),
                (8000, 10, 384, 20), (0, 10, 384, 1), (10, 1 << 31, 384, 1)):
        assert f(*bad) == -1, bad


def _vit_state(seed):
    from ssrl_vit_mae_jepa_amd.classifier import encoder_mae
    m = encoder_mae(TINY)
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in m.encoder.vit.state_dict().items()}


def _assert_loaded(vit, ref):
    got = vit.state_dict()
    assert set(got) == set(ref)
    for k, v in ref.items():
        assert torch.equal(got[k], v), k


def test_checkpoint_layouts_and_loading_mae_family():
    from ssrl_vit_mae_jepa_amd.representation import checkpoint_layout, load_eval_encoder
    vit = _vit_state(1)
    mae_ckpt = {"state_dict": {**{f"model.encoder.vit.{k}": v for k, v in vit.items()}, "model.decoder.decoder_pred.bias": torch.zeros(3)}}
    clf_ckpt = {"state_dict": {**{f"model.encoder.{k}": v for k, v in vit.items()}, "model.head.weight": torch.zeros(10, 32)}}
    mae_pt = {**{f"encoder.vit.{k}": v for k, v in vit.items()}, "encoder.mask_token": torch.zeros(1, 1, 32)}
    for ck, layout, kind in ((mae_ckpt, "mae_ckpt", "mae"), (clf_ckpt, "classifier_ckpt", "classifier"), (mae_pt, "mae_pt", "mae")):
        assert checkpoint_layout(ck.get("state_dict", ck)) == layout
        enc = load_eval_encoder(ck, TINY)
        assert (enc.kind, enc.layout, enc.with_cls) == (kind, layout, True)
        _assert_loaded(enc.vit, vit)
    with pytest.raises(ValueError):
        checkpoint_layout({"foo.bar": torch.zeros(1)})
    with pytest.raises(ValueError):
        load_eval_encoder({"head.weight": torch.zeros(2)}, TINY)
    partial = {k: v for k, v in mae_pt.items() if "blocks.1." not in k}
    with pytest.raises(ValueError, match="missing"):
        load_eval_encoder(partial, TINY)


def test_checkpoint_layouts_and_loading_ijepa():
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    from ssrl_vit_mae_jepa_amd.representation import checkpoint_layout, load_eval_encoder
    cfg = dict(TINY, predictor=dict(pred_embed_dim=32, pred_depth=1, pred_num_heads=2))
    ctx, tgt = _vit_state(2), _vit_state(3)
    # vit-ijepa.pt: context encoder under encoder.vit.*, the EMA encoder under target_encoder.vit.*
    pt = {**{f"encoder.vit.{k}": v for k, v in ctx.items()}, **{f"target_encoder.vit.{k}": v for k, v in tgt.items()}}
    assert checkpoint_layout(pt) == "ijepa_pt"
    for which, ref in (("target", tgt), ("context", ctx)):
        enc = load_eval_encoder(pt, cfg, encoder=which)
        assert (enc.kind, enc.encoder, enc.with_cls) == ("ijepa", which, False)
        _assert_loaded(enc.vit, ref)
    # I-JEPA Lightning checkpoint: model.net.* + model.target_arena
    src = IJEPAPretrainModule(cfg, {})
    with torch.no_grad():
        for name, v in src.model.net.encoder.vit.named_parameters():
            v.copy_(ctx[name])
        views = src.model.target_state_dict()
        for name, v in views.items():
            v.copy_(tgt[name[len("encoder.vit."):]])
    ck = src.checkpoint_dict(0, weights_only=True)
    assert checkpoint_layout(ck["state_dict"]) == "ijepa_ckpt"
    for which, ref in (("target", tgt), ("context", ctx)):
        enc = load_eval_encoder(ck, cfg, encoder=which)
        assert (enc.kind, enc.encoder, enc.with_cls) == ("ijepa", which, False)
        if which == "target":
            got = {k[len("encoder.vit."):]: v for k, v in enc.ijepa.target_state_dict().items()}
        else:
            got = enc.ijepa.net.encoder.vit.state_dict()
        for k, v in ref.items():
            assert torch.equal(got[k], v), (which, k)
    with pytest.raises(ValueError):
        load_eval_encoder(pt, cfg, encoder="ema")


def test_random_encoder_is_the_baseline():
    from ssrl_vit_mae_jepa_amd.classifier import build_baseline_encoder
    from ssrl_vit_mae_jepa_amd.representation import load_eval_encoder
    enc = load_eval_encoder("random", TINY)
    assert enc.kind == "random" and enc.with_cls
    _assert_loaded(enc.vit, build_baseline_encoder(TINY, seed=73).state_dict())


def _ref_normalization(features, mode):  # scripts/evaluation/visualize_representation.py:99-115
    if mode == "none":
        return features
    if mode == "l2":
        return features / (np.linalg.norm(features, axis=1, keepdims=True) + 1e-8)
    mean = features.mean(axis=0, keepdims=True)
    std = features.std(axis=0, keepdims=True) + 1e-8
    return (features - mean) / std


@pytest.mark.parametrize("mode", ["none", "l2", "channel"])
def test_apply_normalization_matches_reference(mode):
    from ssrl_vit_mae_jepa_amd.representation import apply_normalization
    x = np.random.default_rng(0).standard_normal((50, 12)).astype(np.float64) * 3 + 1
    ref = _ref_normalization(x, mode)
    np.testing.assert_array_equal(apply_normalization(x, mode), ref)
    got = apply_normalization(torch.from_numpy(x), mode).numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        apply_normalization(x, "zca")


def test_parse_ks_and_k_larger_than_bank_rejected_before_device_work(tmp_path, monkeypatch):
    from ssrl_vit_mae_jepa_amd.representation import parse_ks
    assert parse_ks("10,20,100,200") == (10, 20, 100, 200)
    assert parse_ks("20, 10,20") == (10, 20)
    for bad in ("", "0", "10,257", "-1"):
        with pytest.raises(ValueError):
            parse_ks(bad)
    from scripts.evaluation import knn_eval
    touched = []
    monkeypatch.setattr(torch.cuda, "is_available", lambda: touched.append(1) or True)
    with pytest.raises(SystemExit, match="exceeds the bank size"):
        knn_eval.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--checkpoint", "random", "--synthetic_images", "50",
                       "--k", "10,60", "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="exceeds the bank size"):
        knn_eval.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--checkpoint", "random", "--synthetic_images", "500",
                       "--samples_per_class", "2", "--k", "21", "--output_dir", str(tmp_path)])
    assert not touched and not list(tmp_path.iterdir())


def test_missing_stl10_files_are_refused(tmp_path, monkeypatch):
    from scripts.evaluation import knn_eval
    monkeypatch.chdir(tmp_path)  # no data/stl10_binary here
    with pytest.raises(SystemExit, match="STL-10 files"):
        knn_eval.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--checkpoint", "random", "--output_dir", str(tmp_path / "o")])
    assert not (tmp_path / "o").exists()


def test_knn_label_shape_checks():
    from ssrl_vit_mae_jepa_amd.representation import knn_classify, knn_vote
    f = torch.zeros(10, 8)
    with pytest.raises(ValueError, match="bank_labels"):
        knn_classify(f, torch.zeros(9, dtype=torch.int64), f, torch.zeros(10, dtype=torch.int64), ks=[1])
    with pytest.raises(ValueError, match="query_labels"):
        knn_classify(f, torch.zeros(10, dtype=torch.int64), f, torch.zeros(11, dtype=torch.int64), ks=[1])
    s, i = torch.zeros(2, 3), torch.tensor([[0, 1, 2], [3, 4, 9]])
    with pytest.raises(ValueError, match="bank_labels"):
        knn_vote(s, i, torch.zeros(9, dtype=torch.int64), 4, bank_size=10)
    with pytest.raises(ValueError, match="past bank_labels"):
        knn_vote(s, i, torch.zeros(9, dtype=torch.int64), 4)


def test_ijepa_config_rejects_cls_pool(tmp_path):
    from scripts.evaluation import knn_eval
    with pytest.raises(SystemExit, match="pool must be mean"):
        knn_eval.main(["--config", str(ROOT / "configs" / "ijepa_vits8.yaml"), "--checkpoint", "random", "--pool", "cls",
                       "--synthetic_images", "50", "--output_dir", str(tmp_path)])


def test_visualize_umap_missing_message():
    try:
        import umap  # noqa: F401
        pytest.skip("umap is installed")
    except ImportError:
        pass
    from scripts.evaluation import visualize_representation as V
    with pytest.raises(RuntimeError, match="UMAP requested but not installed."):
        V.main(["--config", str(ROOT / "configs" / "mae.yaml"), "--encoder_ckpt", "random", "--method", "umap"])
