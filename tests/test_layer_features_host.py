"""Features from any encoder block without a GPU: parse_layers, the two C symbols, every refusal of mae_features_tap and of
mae_engine_extract_layer_features (both return before any HIP call, so made-up addresses are enough), the layer bookkeeping of the
Python API and the new flags and early checks of the evaluation CLIs."""
import ctypes as C
import re
from pathlib import Path

import pytest
import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"
A = 4096   # a made-up, 256-byte aligned device address: no refused call reads it


# ------------------------------------------------------------------------------------------------------------------ parse_layers
@pytest.mark.parametrize("spec,depth,want", [
    ("last", 12, (11,)), ("last", 1, (0,)), ("last1", 12, (11,)), ("last4", 12, (8, 9, 10, 11)), ("last4", 4, (0, 1, 2, 3)), ("LAST2", 12, (10, 11)),
    ("each", 3, (0, 1, 2)), ("each", 1, (0,)), ("2,5,-1", 12, (2, 5, 11)), ("-1,0", 12, (0, 11)), ("5", 12, (5,)), (" 3 , 1 ", 4, (1, 3)),
    ("-12", 12, (0,)), ("11,-2", 12, (10, 11))])
def test_parse_layers(spec, depth, want):
    from ssrl_vit_mae_jepa_amd.representation import parse_layers
    assert parse_layers(spec, depth) == want


@pytest.mark.parametrize("spec,depth", [
    ("last13", 12), ("last0", 12), ("last5", 4), ("lastx", 12), ("last-1", 12), ("first", 12), ("all", 12), ("", 12), ("1,,2", 12), ("1;2", 12),
    ("1.5", 12), ("12", 12), ("-13", 12), ("0,12", 12), ("1,1", 12), ("11,-1", 12), ("0,-12", 12), ("each", 0)])
def test_parse_layers_errors(spec, depth):
    from ssrl_vit_mae_jepa_amd.representation import parse_layers
    with pytest.raises(ValueError):
        parse_layers(spec, depth)


def test_resolve_layers():
    from ssrl_vit_mae_jepa_amd.mae import resolve_layers
    assert resolve_layers([0, 3], 4) == (0, 3) and resolve_layers((-1,), 4) == (3,) and resolve_layers([1, -1], 4) == (1, 3)
    for bad in ([], [3, 1], [1, 1], [4], [-5], [0, -4], [1.5], "13"):
        with pytest.raises(ValueError):
            resolve_layers(bad, 4)


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    raw = HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    for n in ("mae_engine_extract_layer_features", "mae_features_tap"):
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert "MAE_POOL_CLS_MEAN_PATCHES = 3" in raw and _lib.POOL_CLS_MEAN_PATCHES == 3
    assert _lib.ABI_VERSION == 4 and "#define MAE_ABI_VERSION 4" in raw and _lib.lib.mae_abi_version() == 4
    assert len(_lib.SIGNATURES["mae_engine_extract_layer_features"][1]) == 15 and len(_lib.SIGNATURES["mae_features_tap"][1]) == 15


def tap(**kw):
    from ssrl_vit_mae_jepa_amd._lib import lib
    a = dict(x=A, branch=A, dtype=0, gamma=A, beta=A, batch=2, seq=5, dim=8, with_cls=1, pool=1, normalize=0, out=A, stride=8)
    a.update(kw)
    rc = lib.mae_features_tap(a["x"], a["branch"], a["dtype"], a["gamma"], a["beta"], 1e-6, a["batch"], a["seq"], a["dim"], a["with_cls"], a["pool"],
                              a["normalize"], a["out"], a["stride"], None)
    return rc, lib.mae_last_error().decode()


@pytest.mark.parametrize("kw,word", [
    (dict(dim=0), "dim"), (dict(dim=6), "dim"), (dict(dim=1028, stride=1028), "dim"), (dict(dim=-4), "dim"),
    (dict(pool=4), "pool"), (dict(pool=-1), "pool"), (dict(with_cls=2), "with_cls"),
    (dict(pool=0, with_cls=0), "with_cls"), (dict(pool=3, with_cls=0, stride=16), "with_cls"),
    (dict(pool=3, seq=1, stride=16), "seq_len"), (dict(pool=2, seq=1), "seq_len"),
    (dict(stride=4), "out_row_stride"), (dict(stride=10), "out_row_stride"), (dict(pool=3, stride=8), "out_row_stride"), (dict(pool=3, stride=12), "out_row_stride"),
    (dict(out=A + 4), "aligned"), (dict(out=A + 8), "aligned"),
    (dict(dtype=2), "branch_dtype"), (dict(normalize=2), "normalize"), (dict(out=None), "null"), (dict(gamma=None), "null"), (dict(batch=0), "batch")])
def test_features_tap_refuses_before_any_launch(kw, word):
    rc, msg = tap(**kw)
    assert rc != 0 and word in msg and "mae_features_tap" in msg, (kw, msg)


@pytest.fixture(scope="module")
def engine():
    from ssrl_vit_mae_jepa_amd.mae import Engine
    return Engine(dict(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=4, num_heads=2, decoder_embed_dim=64, decoder_depth=1,
                       decoder_num_heads=2), "fp32")


def layer_call(engine, layers, **kw):
    from ssrl_vit_mae_jepa_amd._lib import lib
    a = dict(params=A, images=A, image_dtype=0, batch=2, with_cls=1, pool=0, normalize=0, ws=A, feats=A, n=None, ws_bytes=None)
    a.update(kw)
    need = lib.mae_engine_features_workspace_bytes(engine.handle, 2, 1)
    arr = (C.c_int32 * len(layers))(*layers) if layers is not None else None
    rc = lib.mae_engine_extract_layer_features(engine.handle, a["params"], None, a["images"], a["image_dtype"], a["batch"], a["with_cls"], a["pool"],
                                               a["normalize"], arr, a["n"] if a["n"] is not None else len(layers), a["ws"],
                                               need if a["ws_bytes"] is None else a["ws_bytes"], a["feats"], None)
    return rc, lib.mae_last_error().decode()


@pytest.mark.parametrize("layers,kw,word", [
    ([2, 1], {}, "ascending"), ([1, 1], {}, "ascending"), ([4], {}, "outside"), ([-1], {}, "outside"), ([0, 1, 2, 3, 3], {}, "num_layers"),
    ([0], dict(n=0), "num_layers"), ([0], dict(n=5), "num_layers"), (None, dict(n=1), "null"), ([0], dict(feats=None), "null"),
    ([0], dict(images=None), "null"), ([0], dict(params=None), "null"), ([0], dict(ws=None), "null"),
    ([0], dict(pool=0, with_cls=0), "with_cls"), ([0], dict(pool=3, with_cls=0), "with_cls"), ([0], dict(pool=4), "pool"), ([0], dict(with_cls=2), "with_cls"),
    ([0], dict(normalize=3), "normalize"), ([0], dict(image_dtype=1), "image_dtype"), ([0], dict(ws_bytes=1024), "workspace too small"),
    ([0], dict(feats=A + 4), "aligned")])
def test_engine_call_refuses_before_any_launch(engine, layers, kw, word):
    rc, msg = layer_call(engine, layers, **kw)
    assert rc != 0 and word in msg and "mae_engine_extract_layer_features" in msg, (layers, kw, msg)


def test_old_call_keeps_rejecting_the_new_pool(engine):
    from ssrl_vit_mae_jepa_amd._lib import lib
    need = lib.mae_engine_features_workspace_bytes(engine.handle, 2, 1)
    rc = lib.mae_engine_extract_features(engine.handle, A, None, A, 0, 2, 1, 3, 0, A, need, A, None)
    assert rc != 0 and "pool must be" in lib.mae_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ Python API
TINY = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=3, num_heads=2))


def test_python_api_checks_run_before_the_device():
    from ssrl_vit_mae_jepa_amd.classifier import encoder_mae
    from ssrl_vit_mae_jepa_amd.representation import EvalEncoder, config_depth_dim
    mae = encoder_mae(TINY)
    imgs = torch.zeros(2, 3, 32, 32)
    for kw in (dict(layers=[2, 1]), dict(layers=[1, 1]), dict(layers=[3]), dict(layers=[]), dict(pool="cls_mean"), dict(pool="cls_mean", layers=[0], with_cls=False),
               dict(pool="cls", layers=[0], with_cls=False), dict(pool="nope", layers=[0])):
        with pytest.raises(ValueError):   # _extract: what extract_features runs once it has the arena and the operand copies
            mae._extract(imgs, mae._arena, None, kw.get("pool", "cls"), "none", kw.get("with_cls", True), kw.get("layers"))
    enc = EvalEncoder("mae", "mae_pt", "vit", vit=mae.encoder.vit)
    assert enc.depth == 3 and config_depth_dim(TINY) == (3, 32) and config_depth_dim({}) == (12, 384)
    import inspect
    from ssrl_vit_mae_jepa_amd import representation
    from ssrl_vit_mae_jepa_amd.jepa import IJEPA
    for fn in (EvalEncoder.features, representation.extract_split_features, IJEPA.extract_features):
        assert inspect.signature(fn).parameters["layers"].default is None


# ------------------------------------------------------------------------------------------------------------------ CLIs
def test_cli_parsers_accept_the_new_flags():
    from scripts.evaluation import knn_eval, linear_probe, visualize_representation
    a = knn_eval.parse_args(["--checkpoint", "random", "--layers", "each", "--per_layer", "--pool", "cls_mean"])
    assert (a.layers, a.per_layer, a.pool) == ("each", True, "cls_mean")
    a = knn_eval.parse_args(["--checkpoint", "random"])
    assert (a.layers, a.per_layer) == (None, False)
    a = visualize_representation.parse_args(["--encoder_ckpt", "random", "--layers", "5"])
    assert a.layers == "5" and visualize_representation.parse_args(["--encoder_ckpt", "random"]).layers is None
    a = linear_probe.parse_args(["--checkpoint", "random", "--layers", "last2", "--pool", "cls_mean"])
    assert (a.layers, a.pool) == ("last2", "cls_mean") and linear_probe.parse_args(["--checkpoint", "random"]).layers is None


def _config(tmp_path, encoder):
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["model"]["encoder"] = encoder
    cfg["logging"]["output_dir_base"] = str(tmp_path / "out")
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return path


def test_linear_probe_width_check_fires_before_data_is_loaded(tmp_path, monkeypatch):
    from scripts.evaluation import linear_probe
    path = _config(tmp_path, dict(embed_dim=384, depth=12, num_heads=6))

    def no_data(*a, **k):
        raise AssertionError("data was loaded before the width check")
    monkeypatch.setattr(linear_probe.C, "require_data", no_data)
    monkeypatch.setattr(linear_probe.C, "get_train_batches", no_data)
    with pytest.raises(SystemExit, match="1024"):       # ViT-S last-4: 1536 columns
        linear_probe.main(["--config", str(path), "--checkpoint", "random", "--layers", "last4", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="1024"):       # [cls | mean] of two blocks: 1536 columns
        linear_probe.main(["--config", str(path), "--checkpoint", "random", "--layers", "last2", "--pool", "cls_mean", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="blocks"):
        linear_probe.main(["--config", str(path), "--checkpoint", "random", "--layers", "last13", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="--layers"):
        linear_probe.main(["--config", str(path), "--checkpoint", "random", "--pool", "cls_mean", "--synthetic_images", "50"])
    assert linear_probe.probe_layers("last2", dict(encoder=dict(embed_dim=384, depth=12)), "cls") == ((10, 11), 768)   # ViT-S last-2 fits
    assert linear_probe.probe_layers(None, dict(encoder=dict(embed_dim=384, depth=12)), "cls") == (None, 384)
    with pytest.raises(AssertionError, match="before the width check"):   # a spec that fits goes on to the data
        linear_probe.main(["--config", str(path), "--checkpoint", "random", "--layers", "last2", "--synthetic_images", "50"])


def test_knn_eval_refuses_before_any_device_work(tmp_path, monkeypatch):
    from scripts.evaluation import knn_eval
    path = _config(tmp_path, dict(embed_dim=384, depth=12, num_heads=6))

    def no_data(*a, **k):
        raise AssertionError("data was loaded before the check")
    monkeypatch.setattr(knn_eval, "bank_split", no_data)
    with pytest.raises(SystemExit, match="4096"):       # 12 x 384 = 4608 columns
        knn_eval.main(["--config", str(path), "--checkpoint", "random", "--layers", "each", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="--layers"):
        knn_eval.main(["--config", str(path), "--checkpoint", "random", "--per_layer", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="--layers"):
        knn_eval.main(["--config", str(path), "--checkpoint", "random", "--pool", "cls_mean", "--synthetic_images", "50"])
    with pytest.raises(SystemExit, match="blocks"):
        knn_eval.main(["--config", str(path), "--checkpoint", "random", "--layers", "0,12", "--synthetic_images", "50"])
    with pytest.raises(AssertionError, match="before the check"):   # per layer, every block is fine
        knn_eval.main(["--config", str(path), "--checkpoint", "random", "--layers", "each", "--per_layer", "--synthetic_images", "50"])
