"""Features from any encoder block on the MI355X (mae_engine_extract_layer_features, ``extract_features(layers=...)``): the last
block against the plain call, every block against a truncated model (bit for bit) and against the truncated CPU oracle, subsets and
the early exit, the I-JEPA arenas, refusals, determinism, and the knn_eval / linear_probe CLIs with --layers.

The geometry is MICRO of tests/test_gpu_representation.py (32 px, patch 8, D 48) with four blocks."""
import dataclasses
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from oracle import jepa_oracle as J
from oracle import mae_oracle as O
from tests.knn_ref import pool_ref
from tests.test_gpu_representation import MICRO, POOLS, images_of

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
CFG = dataclasses.replace(MICRO, depth=4)
DEPTH = CFG.depth
LAYER_POOLS = POOLS + [("cls_mean", True)]
_PARAMS = {}


def full_params():
    """The full model's parameters: made once, shared, never modified."""
    if not _PARAMS:
        p = O.init_params(CFG, 73)
        O.randomize_params(p, seed=5)
        _PARAMS.update(p)
    return _PARAMS


def build(dev, precision, depth=DEPTH):
    """The model of the first ``depth`` blocks of the full one, with its embedding and its final norm."""
    from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
    cfg = dataclasses.replace(CFG, depth=depth)
    mae = MaskedAutoencoder(dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
                            dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                            dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads))
    mae.load_state_dict({k: full_params()[k] for k in O.init_params(cfg, 73)})
    return mae.to(dev)


def bits(t):
    return t.contiguous().view(torch.int32)


def width(pool):
    return CFG.embed_dim * (2 if pool == "cls_mean" else 1)


def pooled(ref, pool, norm, with_cls):
    """fp64 reference of a pool, [class | patch mean] included (each half normalised on its own)."""
    if pool == "cls_mean":
        return torch.cat([pool_ref(ref, "cls", norm, True), pool_ref(ref, "mean", norm, True)], dim=1)
    return pool_ref(ref, pool, norm, with_cls)


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("u8", [True, False])
def test_last_block_is_the_plain_feature(dev, precision, u8):
    mae = build(dev, precision)
    imgs = images_of(CFG, 7, u8).to(dev)
    for pool, with_cls in POOLS:
        for norm in ("none", "l2"):
            want = mae.extract_features(imgs, pool=pool, normalize=norm, with_cls=with_cls)
            for layers in ([DEPTH - 1], [-1]):
                got = mae.extract_features(imgs, pool=pool, normalize=norm, with_cls=with_cls, layers=layers)
                assert got.shape == (7, 1, CFG.embed_dim) and got.dtype == torch.float32
                assert torch.equal(bits(got[:, 0]), bits(want)), (pool, with_cls, norm)
    for norm in ("none", "l2"):   # [class | patch mean] = the two plain features side by side
        got = mae.encoder.vit.extract_features(imgs, pool="cls_mean", normalize=norm, layers=[-1])
        want = torch.cat([mae.extract_features(imgs, pool="cls", normalize=norm), mae.extract_features(imgs, pool="mean", normalize=norm)], dim=1)
        assert got.shape == (7, 1, 2 * CFG.embed_dim) and torch.equal(bits(got[:, 0]), bits(want)), norm


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_tap_is_the_truncated_model(dev, precision):
    """Block l of the full model against extract_features of the model of l + 1 blocks: the same kernels on the same shapes."""
    mae = build(dev, precision)
    imgs = images_of(CFG, 9, True).to(dev)
    got = {(pool, wc, norm): mae.extract_features(imgs, pool=pool, normalize=norm, with_cls=wc, layers=range(DEPTH))
           for pool, wc in POOLS for norm in ("none", "l2")}
    for l in range(DEPTH):
        small = build(dev, precision, depth=l + 1)
        for (pool, wc, norm), g in got.items():
            want = small.extract_features(imgs, pool=pool, normalize=norm, with_cls=wc)
            assert torch.equal(bits(g[:, l]), bits(want)), (l, pool, wc, norm, float((g[:, l] - want).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_taps_match_the_truncated_oracle(dev, precision, tol):
    """The bounds of test_extraction_matches_oracle (tests/test_gpu_representation.py), per block."""
    mae, params = build(dev, precision), full_params()
    B, bf = 9, precision == "bf16"
    imgs = images_of(CFG, B, False)
    patches = torch.arange(1, CFG.sequence_length).repeat(B, 1)
    refs = {}
    with torch.no_grad():
        for l in range(DEPTH):
            cfg_l = dataclasses.replace(CFG, depth=l + 1)
            refs[l] = (O.forward_encoder(params, cfg_l, imgs, bf16=bf), O.forward_encoder(params, cfg_l, imgs, idx_keep=patches, bf16=bf))
    worst = 0.0
    for pool, with_cls in LAYER_POOLS:
        for norm in ("none", "l2"):
            got = mae.extract_features(imgs.to(dev), pool=pool, normalize=norm, with_cls=with_cls, layers=list(range(DEPTH))).double().cpu()
            assert got.shape == (B, DEPTH, width(pool))
            for l in range(DEPTH):
                ref = pooled(refs[l][0 if with_cls else 1], pool, norm, with_cls)
                err = float((got[:, l] - ref).abs().max())
                bound = (3 * 2.0 ** -8 if bf else tol) * float(ref.abs().max())
                worst = max(worst, err / bound)
                if bf:
                    assert float((got[:, l] - ref).norm() / ref.norm()) <= tol, (l, pool, with_cls, norm)
                assert err <= bound, (l, pool, with_cls, norm, err)
    print(f"{precision}: worst error / bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_subsets_and_early_exit(dev, precision):
    mae = build(dev, precision)
    imgs = images_of(CFG, 5, True).to(dev)
    for pool, norm in (("mean", "l2"), ("cls_mean", "none")):
        each = mae.extract_features(imgs, pool=pool, normalize=norm, layers=range(DEPTH))
        one = mae.extract_features(imgs, pool=pool, normalize=norm, layers=[1])
        two = mae.extract_features(imgs, pool=pool, normalize=norm, layers=[1, 3])
        neg = mae.extract_features(imgs, pool=pool, normalize=norm, layers=[-3, -1])
        assert one.shape == (5, 1, width(pool)) and two.shape == (5, 2, width(pool))
        assert torch.equal(bits(one[:, 0]), bits(each[:, 1])) and torch.equal(bits(two[:, 0]), bits(each[:, 1]))
        assert torch.equal(bits(two[:, 1]), bits(each[:, 3])) and torch.equal(bits(neg), bits(two))
    # a call for block 1 launches the kernels of two blocks: the engine's timers count one attention launch per block
    mae.engine.timers_enable(True)
    mae.engine.timers_reset()
    mae.extract_features(imgs, layers=[1])
    torch.cuda.synchronize()
    t = mae.engine.timers_read()
    mae.engine.timers_enable(False)
    assert t["attention_fwd"]["launches"] == 2, t


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_ijepa_target_and_context_taps(dev, precision, tol):
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    cfg, B = dataclasses.replace(J.JEPA_MICRO, depth=3), 4
    mc = dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
              encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
              predictor=dict(pred_embed_dim=cfg.pred_embed_dim, pred_depth=cfg.pred_depth, pred_num_heads=cfg.pred_num_heads))
    module = IJEPAPretrainModule(mc, dict(total_epochs=10, warmup_epochs=1, steps_per_epoch=4, batch_size=512, ema_start=0.5, ema_end=1.0))
    params = J.init_params(cfg, 73)
    J.M.randomize_params(params)
    module.model.net.load_state_dict(params)
    module.model.reset_target()
    module = module.to(dev)
    for step in (1, 2):   # the two arenas part
        images = J.M.synthetic_images(B, cfg.as_mae(), seed=100 + step)
        ctx, tgt = J.sample_masks(cfg, B, torch.Generator().manual_seed(step))
        module.fused_training_step(images.to(dev), ctx, tgt, lr=1e-2)
    model = module.model
    imgs = J.M.synthetic_images(6, cfg.as_mae(), seed=9)
    ctx_p = {k: v.detach().cpu() for k, v in model.net.state_dict().items()}
    tgt_p = dict(ctx_p, **{k: v.detach().cpu() for k, v in model.target_state_dict().items()})
    patches = torch.arange(1, cfg.num_patches + 1).repeat(imgs.shape[0], 1)
    bf = precision == "bf16"
    for which, p in (("target", tgt_p), ("context", ctx_p)):
        got = model.extract_features(imgs.to(dev), encoder=which, layers=range(cfg.depth))
        assert got.shape == (6, cfg.depth, cfg.embed_dim)
        assert torch.equal(bits(got[:, -1]), bits(model.extract_features(imgs.to(dev), encoder=which)))
        l2 = model.extract_features(imgs.to(dev), encoder=which, normalize="l2", layers=[0, 2]).double().cpu()
        for l in range(cfg.depth):
            with torch.no_grad():
                ref = J.encode_tokens(p, dataclasses.replace(cfg, depth=l + 1), imgs, patches, bf16=bf).double().mean(1)
            g = got[:, l].double().cpu()
            if bf:
                assert float((g - ref).norm() / ref.norm()) <= tol, (which, l)
            assert float((g - ref).abs().max()) <= (3 * 2.0 ** -8 if bf else tol) * float(ref.abs().max()), (which, l)
            if l in (0, 2):
                assert torch.allclose(l2[:, l // 2], g / (g.norm(dim=1, keepdim=True) + 1e-8), rtol=1e-5, atol=1e-6)
    t = model.extract_features(imgs.to(dev), encoder="target", layers=[1])
    c = model.extract_features(imgs.to(dev), encoder="context", layers=[1])
    assert not torch.equal(t, c)
    with pytest.raises(ValueError):
        model.extract_features(imgs.to(dev), pool="cls_mean", layers=[1])


# ------------------------------------------------------------------------------------------------------------------ 6, 7
def test_refusals(dev):
    import ctypes as C

    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    mae = build(dev, "fp32")
    imgs = images_of(CFG, 3, False).to(dev)
    for kw in (dict(layers=[2, 1]), dict(layers=[1, 1]), dict(layers=[DEPTH]), dict(layers=[-DEPTH - 1]), dict(layers=[]),
               dict(pool="cls_mean", with_cls=False, layers=[1]), dict(pool="cls", with_cls=False, layers=[1]), dict(pool="cls_mean")):
        with pytest.raises(ValueError):
            mae.extract_features(imgs, **kw)
    # the engine's own refusals: nothing is written
    need = lib.mae_engine_features_workspace_bytes(mae.engine.handle, 3, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((3, 2, 2 * CFG.embed_dim), float("nan"), device=dev)

    def call(layers, with_cls=1, pool=_lib.POOL_CLS, ws_bytes=need):
        rc = lib.mae_engine_extract_layer_features(mae.engine.handle, _ptr(mae.flat_params), None, _ptr(imgs), _lib.MAE_F32, 3, with_cls, pool, 0,
                                                   (C.c_int32 * len(layers))(*layers), len(layers), _ptr(ws), ws_bytes, _ptr(out), _stream(dev))
        _lib.check(0)
        return rc, lib.mae_last_error().decode()
    for args, word in ((dict(layers=[2, 1]), "ascending"), (dict(layers=[1, 1]), "ascending"), (dict(layers=[0, DEPTH]), "outside"),
                       (dict(layers=[1], with_cls=0, pool=_lib.POOL_CLS_MEAN_PATCHES), "with_cls"), (dict(layers=[1], ws_bytes=need - 1), "workspace too small")):
        rc, msg = call(**args)
        assert rc != 0 and word in msg, (args, msg)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    rc, msg = call([1, 3])
    assert rc == 0, msg
    torch.cuda.synchronize()
    n = 3 * 2 * CFG.embed_dim                                   # (3, 2, D) packed at the front of the buffer
    assert torch.isfinite(out.view(-1)[:n]).all() and torch.isnan(out.view(-1)[n:]).all()


def test_determinism_and_no_autograd_graph(dev):
    mae = build(dev, "bf16")
    imgs = images_of(CFG, 16, True).to(dev)
    a = mae.extract_features(imgs, pool="cls_mean", normalize="l2", layers=range(DEPTH))
    b = mae.extract_features(imgs, pool="cls_mean", normalize="l2", layers=range(DEPTH))
    assert torch.equal(bits(a), bits(b))
    assert not a.requires_grad and a.grad_fn is None and a.dtype == torch.float32 and a.is_contiguous()
    norms = a.view(16, DEPTH, 2, CFG.embed_dim).double().norm(dim=-1)   # every (layer, pool) slice is a unit vector
    assert float((norms - 1).abs().max()) < 1e-5
    out = mae.encoder.vit.forward_features(imgs)               # records the encoder's autograd node
    mae.extract_features(imgs, layers=[0])                     # overwrites the saved activations
    with pytest.raises(RuntimeError, match="overwrote"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------------------------ 8
def _run(*a):
    return subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_knn_eval_per_layer_cli(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["model"]["encoder"] = dict(embed_dim=48, depth=4, num_heads=2)
    cfg["model"].pop("decoder", None)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    common = ["scripts.evaluation.knn_eval", "--config", str(path), "--checkpoint", "random", "--synthetic_images", "200", "--k", "10,20", "--batch_size", "100"]
    r = _run(*common, "--layers", "each", "--per_layer", "--output_dir", str(tmp_path / "a"))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert json.loads((tmp_path / "a" / "knn.json").read_text()) == res
    assert res["layers"] == [0, 1, 2, 3] and set(res["per_layer"]) == {"0", "1", "2", "3"}
    assert all(set(v) == {"10", "20"} and all(0.0 <= x <= 1.0 for x in v.values()) for v in res["per_layer"].values())
    r = _run(*common, "--output_dir", str(tmp_path / "b"))
    assert r.returncode == 0, r.stderr[-3000:]
    plain = json.loads(r.stdout.strip().splitlines()[-1])
    assert "layers" not in plain and "per_layer" not in plain
    assert res["per_layer"]["3"] == plain["top1"] == res["top1"]
    r = _run(*common, "--layers", "last2", "--pool", "cls_mean", "--output_dir", str(tmp_path / "c"))   # the concatenation: (N, 2 * 96)
    assert r.returncode == 0, r.stderr[-3000:]
    cat = json.loads(r.stdout.strip().splitlines()[-1])
    assert cat["layers"] == [2, 3] and "per_layer" not in cat and set(cat["top1"]) == {"10", "20"}


def test_linear_probe_layers_cli(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "vits8_dec192_linprobe.yaml").read_text())
    cfg["model"]["encoder"] = dict(embed_dim=48, depth=4, num_heads=2)
    cfg["model"].pop("decoder", None)
    cfg.setdefault("logging", {})["output_dir_base"] = str(tmp_path / "out")
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    common = ["scripts.evaluation.linear_probe", "--config", str(path), "--checkpoint", "random", "--synthetic_images", "200", "--batch_size", "64"]
    r = _run(*common, "--layers", "last2", "--max_epochs", "2")
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "out" / "probe" / "linprobe"
    res = json.loads((out / "probe.json").read_text())
    assert res["layers"] == [2, 3] and res["epochs"] == 2 and 0.0 <= res["test_acc"] <= 1.0
    assert not (out / "checkpoints" / "best.ckpt").exists() and not (out / "checkpoints" / "last.ckpt").exists()
    state = torch.load(out / "checkpoints" / "probe_last.pt", map_location="cpu", weights_only=False)
    assert state["layers"] == [2, 3] and state["head.classification.classification.weight"].shape[1] == 96
    r = _run(*common, "--layers", "last", "--max_epochs", "1", "--resume", str(out / "checkpoints" / "probe_last.pt"))
    assert r.returncode != 0 and "layers" in r.stderr
