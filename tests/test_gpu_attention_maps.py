"""Attention maps of the encoder on the MI355X (mae_engine_extract_attention, ``extract_attention``): shapes and sums, every block against
the truncated model (bit for bit), subsets and the early exit, the CPU oracle walk of the same precision, the I-JEPA arenas,
``EvalEncoder.attention``, refusals, and the visualize_attention CLI.

The geometry is MICRO of tests/test_gpu_representation.py with four blocks, as tests/test_gpu_layer_features.py: L = 17, H = 2, hd = 24.

The oracle comparison has no fixed tolerance.  The engine runs the same fp32 or bf16 operations as the oracle in another order, so
agreement means a small multiple K of the oracle's own distance from fp64, max |walk(precision) - walk(fp64)| per block, which the test
computes on the CPU from the same inputs.  Measured (printed with -s), worst over blocks and queries: fp32 maps 1.61, rollout 1.82,
I-JEPA maps 2.95; bf16 maps 1.18, rollout 0.90.  K = 8: the noise is that of the host's fp32 sums, whose order differs between CPUs,
so the allowance is the start value 4, which held, doubled once against another host's oracle."""
import ctypes as C
import dataclasses
import json
import subprocess
import sys

import pytest
import torch

from oracle import jepa_oracle as J
from tests import attnmap_ref as R
from tests.test_gpu_layer_features import CFG, DEPTH, ROOT, bits, build, full_params
from tests.test_gpu_representation import images_of

pytestmark = pytest.mark.gpu

K = 8   # multiple of the oracle's own rounding noise the engine may differ by (module docstring); never above 16
B = 9
L, H = CFG.sequence_length, CFG.num_heads
QUERIES = (("cls", True), ("mean", True), ("mean", False))


# ------------------------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("u8", [True, False])
def test_shapes_sums_and_no_graph(dev, precision, u8):
    mae = build(dev, precision)
    imgs = images_of(CFG, B, u8).to(dev)
    for query, with_cls in QUERIES:
        T = L if with_cls else L - 1
        maps = mae.extract_attention(imgs, layers=range(DEPTH), query=query, with_cls=with_cls)
        assert maps.shape == (B, DEPTH, H, T) and maps.dtype == torch.float32 and maps.is_contiguous()
        assert not maps.requires_grad and maps.grad_fn is None
        assert bool((maps >= 0).all()) and float((maps.double().sum(-1) - 1).abs().max()) <= 1e-5
        m2, roll = mae.extract_attention(imgs, layers=range(DEPTH), query=query, with_cls=with_cls, rollout=True)
        assert torch.equal(bits(m2), bits(maps))                   # the rollout changes no map, and two runs agree bit for bit
        assert roll.shape == (B, T) and roll.dtype == torch.float32 and not roll.requires_grad
        assert bool((roll > 0).all()) and float((roll.double().sum(-1) - 1).abs().max()) <= 1e-5
    last = mae.extract_attention(imgs)                             # the defaults: the class-token maps of the last block
    assert torch.equal(bits(last), bits(mae.encoder.vit.extract_attention(imgs, layers=[DEPTH - 1], query="cls")))
    assert last.shape == (B, 1, H, L)


# ------------------------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_every_block_is_the_truncated_model(dev, precision):
    """Block l of the full model against the last block of the model of l + 1 blocks: the same kernels on the same shapes."""
    mae = build(dev, precision)
    imgs = images_of(CFG, B, True).to(dev)
    got = {q: mae.extract_attention(imgs, layers=range(DEPTH), query=q[0], with_cls=q[1]) for q in QUERIES}
    rolls = {(q, l): mae.extract_attention(imgs, layers=[l], query=q[0], with_cls=q[1], rollout=True) for q in QUERIES for l in range(DEPTH)}
    for l in range(DEPTH):
        small = build(dev, precision, depth=l + 1)
        for q in QUERIES:
            want, want_roll = small.extract_attention(imgs, layers=[-1], query=q[0], with_cls=q[1], rollout=True)
            assert torch.equal(bits(got[q][:, l]), bits(want[:, 0])), (l, q)
            m, r = rolls[q, l]
            assert torch.equal(bits(m), bits(want)) and torch.equal(bits(r), bits(want_roll)), (l, q)


# ------------------------------------------------------------------------------------------------------------------ 3, 4
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_subsets_and_early_exit(dev, precision):
    mae = build(dev, precision)
    imgs = images_of(CFG, 5, True).to(dev)
    for query, with_cls in QUERIES:
        kw = dict(query=query, with_cls=with_cls)
        each, roll_each = mae.extract_attention(imgs, layers=range(DEPTH), rollout=True, **kw)
        one = mae.extract_attention(imgs, layers=[1], **kw)
        two, roll_two = mae.extract_attention(imgs, layers=[1, 3], rollout=True, **kw)
        neg = mae.extract_attention(imgs, layers=[-3, -1], **kw)
        assert one.shape == (5, 1, H, each.shape[-1]) and two.shape == (5, 2, H, each.shape[-1])
        assert torch.equal(bits(one[:, 0]), bits(each[:, 1])) and torch.equal(bits(two[:, 0]), bits(each[:, 1]))
        assert torch.equal(bits(two[:, 1]), bits(each[:, 3])) and torch.equal(bits(neg), bits(two))
        assert torch.equal(bits(roll_two), bits(roll_each))        # the rollout runs from block 3 to block 0 whatever else is listed
    # A call for block 1 runs two blocks.  The engine's timers count, per block, one attention launch and four Linear launches (one more
    # for the patch embedding); the map kernel is timed as attention too: one launch for the map, one more for the second rollout step.
    mae.engine.timers_enable(True)
    for rollout, attn in ((False, 2 + 1), (True, 2 + 2)):
        mae.engine.timers_reset()
        mae.extract_attention(imgs, layers=[1], rollout=rollout)
        torch.cuda.synchronize()
        t = mae.engine.timers_read()
        assert t["attention_fwd"]["launches"] == attn and t["linear_nt"]["launches"] == 1 + 2 * 4, t
        assert t["attention_fwd"]["flops"] > 0 and t["attention_fwd"]["bytes"] > 0
    mae.engine.timers_enable(False)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_block_0_alone_is_slice_0_of_every_block(dev, precision):
    """The earliest stop: maps and features for layers=[0] hold the bits of slice 0 of the call for every block, from one block's launches."""
    mae = build(dev, precision)
    imgs = images_of(CFG, 3, True).to(dev)
    for query, with_cls in QUERIES:
        each = mae.extract_attention(imgs, layers=range(DEPTH), query=query, with_cls=with_cls)
        first = mae.extract_attention(imgs, layers=[0], query=query, with_cls=with_cls)
        assert first.shape == (3, 1, H, each.shape[-1]) and torch.equal(bits(first[:, 0]), bits(each[:, 0])), (query, with_cls)
    for pool, norm in (("mean", "l2"), ("cls_mean", "none")):
        each = mae.extract_features(imgs, pool=pool, normalize=norm, layers=range(DEPTH))
        first = mae.extract_features(imgs, pool=pool, normalize=norm, layers=[0])
        assert first.shape == (3, 1, each.shape[-1]) and torch.equal(bits(first[:, 0]), bits(each[:, 0])), (pool, norm)
    mae.engine.timers_enable(True)
    for call, attn in ((lambda: mae.extract_attention(imgs, layers=[0]), 1 + 1), (lambda: mae.extract_features(imgs, layers=[0]), 1)):
        mae.engine.timers_reset()
        call()
        torch.cuda.synchronize()
        t = mae.engine.timers_read()
        assert t["attention_fwd"]["launches"] == attn and t["linear_nt"]["launches"] == 1 + 4, t   # the patch embedding and one block
    mae.engine.timers_enable(False)


# ------------------------------------------------------------------------------------------------------------------ 5
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_maps_and_rollout_match_the_oracle_walk(dev, precision):
    mae, params = build(dev, precision), full_params()
    bf = precision == "bf16"
    imgs = images_of(CFG, B, False)
    worst = {}
    for query, with_cls in QUERIES:
        with torch.no_grad():
            walk = R.oracle_walk(params, CFG, imgs, with_cls, bf)
            walk64 = R.walk_fp64(params, CFG, imgs, with_cls)
        layers = list(range(DEPTH))
        ref, ref64 = R.maps_of(walk, query, layers), R.maps_of(walk64, query, layers)
        w = R.start_weight(query, B, ref.shape[-1])
        roll_ref, roll64 = R.rollout_ref(walk, w), R.rollout_ref(walk64, w)
        got, roll = mae.extract_attention(imgs.to(dev), layers=layers, query=query, with_cls=with_cls, rollout=True)
        got, roll = got.double().cpu(), roll.double().cpu()
        for l in layers:
            noise = float((ref[:, l] - ref64[:, l]).abs().max())
            err = float((got[:, l] - ref[:, l]).abs().max())
            print(f"{precision} {query} with_cls={with_cls} block {l}: maps in [{float(ref[:, l].min()):.3g}, {float(ref[:, l].max()):.3g}], "
                  f"oracle noise {noise:.3g}, engine - oracle {err:.3g}, ratio {err / noise:.2f}")
            worst["maps"] = max(worst.get("maps", 0.0), err / noise)
            assert noise > 0 and err <= K * noise, (query, with_cls, l, err, noise)
        noise = float((roll_ref - roll64).abs().max())
        err = float((roll - roll_ref).abs().max())
        print(f"{precision} {query} with_cls={with_cls} rollout: oracle noise {noise:.3g}, engine - oracle {err:.3g}, ratio {err / noise:.2f}")
        worst["rollout"] = max(worst.get("rollout", 0.0), err / noise)
        assert noise > 0 and err <= K * noise, (query, with_cls, "rollout", err, noise)
    print(f"{precision}: worst (engine - oracle) / oracle noise: maps {worst['maps']:.2f}, rollout {worst['rollout']:.2f} (allowed {K})")


# ------------------------------------------------------------------------------------------------------------------ 6, 7
def jepa_module(dev, precision, depth=3):
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    cfg = dataclasses.replace(J.JEPA_MICRO, depth=depth)
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
        images = J.M.synthetic_images(4, cfg.as_mae(), seed=100 + step)
        ctx, tgt = J.sample_masks(cfg, 4, torch.Generator().manual_seed(step))
        module.fused_training_step(images.to(dev), ctx, tgt, lr=1e-2)
    return module, cfg


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_ijepa_target_and_context_maps(dev, precision):
    module, cfg = jepa_module(dev, precision)
    model = module.model
    imgs = J.M.synthetic_images(6, cfg.as_mae(), seed=9)
    N = cfg.num_patches                                               # 64 patch tokens: one full lane row, no tail
    ctx_p = {k: v.detach().cpu() for k, v in model.net.state_dict().items()}
    tgt_p = dict(ctx_p, **{k: v.detach().cpu() for k, v in model.target_state_dict().items()})
    out = {}
    for which, p in (("target", tgt_p), ("context", ctx_p)):
        maps, roll = model.extract_attention(imgs.to(dev), encoder=which, layers=range(cfg.depth), rollout=True)
        assert maps.shape == (6, cfg.depth, cfg.num_heads, N) and roll.shape == (6, N)
        assert float((maps.double().sum(-1) - 1).abs().max()) <= 1e-5 and float((roll.double().sum(-1) - 1).abs().max()) <= 1e-5
        assert torch.equal(bits(maps[:, -1:]), bits(model.extract_attention(imgs.to(dev), encoder=which)))   # the default: the last block
        with torch.no_grad():
            walk = R.oracle_walk(p, cfg.as_mae(), imgs, False, precision == "bf16")
            walk64 = R.walk_fp64(p, cfg.as_mae(), imgs, False)
        ref, ref64 = R.maps_of(walk, "mean", range(cfg.depth)), R.maps_of(walk64, "mean", range(cfg.depth))
        for l in range(cfg.depth):
            noise = float((ref[:, l] - ref64[:, l]).abs().max())
            err = float((maps[:, l].double().cpu() - ref[:, l]).abs().max())
            print(f"{precision} {which} block {l}: oracle noise {noise:.3g}, engine - oracle {err:.3g}, ratio {err / noise:.2f}")
            assert err <= K * noise, (which, l, err, noise)
        w = R.start_weight("mean", 6, N)
        noise = float((R.rollout_ref(walk, w) - R.rollout_ref(walk64, w)).abs().max())
        err = float((roll.double().cpu() - R.rollout_ref(walk, w)).abs().max())
        print(f"{precision} {which} rollout: oracle noise {noise:.3g}, engine - oracle {err:.3g}, ratio {err / noise:.2f}")
        assert err <= K * noise, (which, "rollout", err, noise)
        out[which] = maps
    assert not torch.equal(out["target"], out["context"])
    for kw in (dict(query="cls"), dict(encoder="teacher"), dict(layers=[cfg.depth])):
        with pytest.raises(ValueError):
            model.extract_attention(imgs.to(dev), **kw)


def test_eval_encoder_attention(dev):
    from ssrl_vit_mae_jepa_amd.representation import EvalEncoder, attention_grid
    mae = build(dev, "bf16")
    imgs = images_of(CFG, 5, True).to(dev)
    enc = EvalEncoder("mae", "mae_pt", "vit", vit=mae.encoder.vit)
    maps, roll = enc.attention(imgs, layers=[1, 3], rollout=True)       # query defaults to the class token
    want = mae.extract_attention(imgs, layers=[1, 3], query="cls", rollout=True)
    assert torch.equal(bits(maps), bits(want[0])) and torch.equal(bits(roll), bits(want[1]))
    assert torch.equal(bits(enc.attention(imgs, query="mean")), bits(mae.extract_attention(imgs, query="mean")))
    grid = attention_grid(maps, True, CFG.image_size // CFG.patch_size)
    assert grid.shape == (5, 2, H, 4, 4) and float((grid.double().sum((-1, -2)) - 1).abs().max()) <= 1e-5
    mae.encoder.vit.with_cls = False                                      # a classifier fine-tuned from I-JEPA: patch tokens only
    try:
        assert torch.equal(bits(enc.attention(imgs)), bits(mae.extract_attention(imgs, query="mean", with_cls=False)))
        with pytest.raises(ValueError):
            enc.attention(imgs, query="cls")
    finally:
        mae.encoder.vit.with_cls = True
    module, cfg = jepa_module(dev, "bf16")
    jimgs = J.M.synthetic_images(4, cfg.as_mae(), seed=9).to(dev)
    for which in ("target", "context"):
        enc = EvalEncoder("ijepa", "ijepa_ckpt", which, ijepa=module.model)
        assert not enc.with_cls
        maps, roll = enc.attention(jimgs, layers=range(cfg.depth), rollout=True)
        want = module.model.extract_attention(jimgs, encoder=which, layers=range(cfg.depth), rollout=True)
        assert torch.equal(bits(maps), bits(want[0])) and torch.equal(bits(roll), bits(want[1]))
        assert attention_grid(roll, False, cfg.grid).shape == (4, cfg.grid, cfg.grid)


# ------------------------------------------------------------------------------------------------------------------ 8
def test_refusals(dev):
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    mae = build(dev, "fp32")
    imgs = images_of(CFG, 3, False).to(dev)
    for kw in (dict(layers=[2, 1]), dict(layers=[1, 1]), dict(layers=[DEPTH]), dict(layers=[]), dict(query="cls", with_cls=False), dict(query="max")):
        with pytest.raises(ValueError):
            mae.extract_attention(imgs, **kw)
    need = lib.mae_engine_attention_workspace_bytes(mae.engine.handle, 3, 1)
    assert need == lib.mae_engine_features_workspace_bytes(mae.engine.handle, 3, 1) > 0
    assert lib.mae_engine_attention_workspace_bytes(mae.engine.handle, 0, 1) < 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    maps = torch.full((3, 2, H, L), float("nan"), device=dev)
    roll = torch.full((3, L), float("nan"), device=dev)

    def call(layers, with_cls=1, query=_lib.ATTN_QUERY_CLS, ws_bytes=need, m=maps, r=roll):
        rc = lib.mae_engine_extract_attention(mae.engine.handle, _ptr(mae.flat_params), None, _ptr(imgs), _lib.MAE_F32, 3, with_cls, query,
                                              (C.c_int32 * len(layers))(*layers), len(layers), _ptr(m), _ptr(r), _ptr(ws), ws_bytes, _stream(dev))
        _lib.check(0)
        return rc, lib.mae_last_error().decode()
    for args, word in ((dict(layers=[2, 1]), "ascending"), (dict(layers=[0, DEPTH]), "outside"), (dict(layers=[1], with_cls=0), "with_cls"),
                       (dict(layers=[1], query=2), "query"), (dict(layers=[1], m=None, r=None), "null"), (dict(layers=[1], ws_bytes=need - 1), "workspace too small"),
                       (dict(layers=[1], r=roll.view(-1)[1:]), "aligned")):
        rc, msg = call(**args)
        assert rc != 0 and word in msg, (args.keys(), msg)
    torch.cuda.synchronize()
    assert torch.isnan(maps).all() and torch.isnan(roll).all()
    rc, msg = call([1, 3], m=None)                                  # the rollout alone
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.isnan(maps).all() and torch.isfinite(roll).all()
    rc, msg = call([1, 3], r=None)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert torch.isfinite(maps).all()
    want, want_roll = mae.extract_attention(imgs, layers=[1, 3], rollout=True)
    assert torch.equal(bits(maps), bits(want)) and torch.equal(bits(roll), bits(want_roll))


def test_overwrites_a_pending_backward(dev):
    mae = build(dev, "bf16")
    imgs = images_of(CFG, 4, True).to(dev)
    out = mae.encoder.vit.forward_features(imgs)               # records the encoder's autograd node
    mae.extract_attention(imgs, layers=[0])                    # overwrites the saved activations
    with pytest.raises(RuntimeError, match="overwrote"):
        out.sum().backward()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_visualize_attention_cli(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["model"]["encoder"] = dict(embed_dim=48, depth=4, num_heads=2)
    cfg["model"].pop("decoder", None)
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, "-m", "scripts.evaluation.visualize_attention", "--config", str(path), "--checkpoint", "random", "--synthetic_images", "16",
                        "--num_samples", "4", "--layers", "each", "--rollout", "--output_dir", str(tmp_path / "out")],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads((tmp_path / "out" / "attention.json").read_text())
    assert json.loads(r.stdout.strip().splitlines()[-1]) == res
    assert res["layers"] == [0, 1, 2, 3] and res["query"] == "cls" and res["with_cls"] is True and res["heads"] == 2 and res["images"] >= 4
    T = res["tokens"]
    assert res["uniform_entropy"] == pytest.approx(float(torch.log(torch.tensor(float(T), dtype=torch.float64))))
    assert set(res["blocks"]) == {"0", "1", "2", "3"}
    for blk in res["blocks"].values():
        assert len(blk["entropy"]) == 2 and all(0.0 <= e <= res["uniform_entropy"] + 1e-9 for e in blk["entropy"])
        assert len(blk["class_mass"]) == 2 and all(0.0 < m < 1.0 for m in blk["class_mass"])
    assert res["rollout"]["from_block"] == 3 and 0.0 < res["rollout"]["class_mass"] < 1.0
    fig = tmp_path / "out" / res["figure"].split("/")[-1]
    assert fig.suffix == ".png" and fig.stat().st_size > 10_000
