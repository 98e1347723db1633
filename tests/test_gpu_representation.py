"""Frozen-encoder features and the k-NN probe on the MI355X: extraction against forward_features and the CPU oracle,
I-JEPA target / context encoders, a full-size run, top-k and vote against fp64, ties, NaN, split invariance,
self-retrieval and the knn_eval CLI."""
import json
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from oracle import jepa_oracle as J
from oracle import mae_oracle as O
from tests.knn_ref import check_topk, pool_ref, topk_ref, vote_ref

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def build_mae(dev, precision, cfg=MICRO, seed=5):
    from ssrl_vit_mae_jepa_amd import MaskedAutoencoder
    mae = MaskedAutoencoder(dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
                            dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                            dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads))
    params = O.init_params(cfg, 73)
    O.randomize_params(params, seed=seed)
    mae.load_state_dict(params)
    return mae.to(dev), params


def images_of(cfg, B, u8, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, cfg.in_chans, cfg.image_size, cfg.image_size), dtype=torch.uint8, generator=g)
    return x if u8 else (x.float() / 255 - 0.5) / 0.5


POOLS = [("cls", True), ("mean", True), ("mean_all", True), ("mean", False), ("mean_all", False)]


# ------------------------------------------------------------------------------------------------------------------
# feature extraction
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("u8", [True, False])
@pytest.mark.parametrize("B", [7, 33])
def test_extraction_matches_forward_features(dev, precision, u8, B):
    mae, _ = build_mae(dev, precision)
    imgs = images_of(MICRO, B, u8).to(dev)
    with torch.no_grad():
        full = mae.encoder.vit.forward_features(imgs)             # (B, L, D) fp32, [cls | patches]
    for pool, with_cls in POOLS:
        if not with_cls:
            continue
        for norm in ("none", "l2"):
            got = mae.extract_features(imgs, pool=pool, normalize=norm, with_cls=with_cls)
            assert got.shape == (B, MICRO.embed_dim) and got.dtype == torch.float32 and not got.requires_grad
            ref = pool_ref(full.cpu(), pool, norm)
            err = float((got.double().cpu() - ref).abs().max())
            assert err <= 1e-5 * float(ref.abs().max()), (pool, norm, err)
    via_vit = mae.encoder.vit.extract_features(imgs, pool="mean", normalize="l2")
    assert torch.equal(via_vit, mae.extract_features(imgs, pool="mean", normalize="l2"))


# fp32: max|d| <= 1e-4 max|ref|.  bf16: relative norm <= 2e-2 (the bound of the classifier's bf16 feature tests) and max|d| <=
# 3 bf16 units (2^-8) of max|ref|; see the comment in the test
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_extraction_matches_oracle(dev, precision, tol):
    mae, params = build_mae(dev, precision)
    B = 9
    imgs = images_of(MICRO, B, False)
    bf = precision == "bf16"
    with torch.no_grad():
        ref_cls = O.forward_encoder(params, MICRO, imgs, bf16=bf)
        patches = torch.arange(1, MICRO.sequence_length).repeat(B, 1)
        ref_nocls = O.forward_encoder(params, MICRO, imgs, idx_keep=patches, bf16=bf)
    for pool, with_cls in POOLS:
        for norm in ("none", "l2"):
            got = mae.extract_features(imgs.to(dev), pool=pool, normalize=norm, with_cls=with_cls).double().cpu()
            ref = pool_ref(ref_cls if with_cls else ref_nocls, pool, norm, with_cls)
            err = float((got - ref).abs().max())
            if bf:
                # bf16: the encoder's blocks round their GEMM operands where the oracle does, but an fp32 sum that lands on the
                # other side of a bf16 rounding boundary flips one unit (2^-8) there, and the flips propagate through the
                # blocks.  A single class-token row shows them per element: measured max 6.7e-3 of max|ref| (1.7 units) at
                # this size, above the 5e-3 the loss tests apply to a mean over every element.  The bound here is the
                # classifier feature tests' relative norm (tol) plus 3 units per element.  The fused final step itself is
                # checked against the engine's own forward_features at 1e-5 above, so none of this comes from it.
                assert float((got - ref).norm() / ref.norm()) <= tol, (pool, with_cls, norm)
                assert err <= 3 * 2.0 ** -8 * float(ref.abs().max()), (pool, with_cls, norm, err)
            else:
                assert err <= tol * float(ref.abs().max()), (pool, with_cls, norm, err)
    with pytest.raises(ValueError):
        mae.extract_features(imgs.to(dev), pool="cls", with_cls=False)


def test_extraction_is_deterministic_and_guards_backward(dev):
    mae, _ = build_mae(dev, "bf16")
    imgs = images_of(MICRO, 16, True).to(dev)
    a = mae.extract_features(imgs, pool="mean", normalize="l2")
    b = mae.extract_features(imgs, pool="mean", normalize="l2")
    assert torch.equal(a, b)
    out = mae.encoder.vit.forward_features(imgs)               # records the encoder's autograd node
    mae.extract_features(imgs)                                 # overwrites the saved activations
    with pytest.raises(RuntimeError, match="overwrote"):
        out.sum().backward()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_plain_call_takes_a_4_byte_aligned_feats(dev, precision):
    """mae_engine_extract_features writes wherever a float may start: feats one float into a NaN-filled buffer gives the bits of the
    aligned call and leaves the floats around the written range NaN.  (The 16-byte rule belongs to the layer call alone.)"""
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import FEATURE_NORMS, FEATURE_POOLS, _ptr, _stream
    mae, _ = build_mae(dev, precision)
    B, D = 3, MICRO.embed_dim
    imgs = images_of(MICRO, B, True).to(dev)
    need = lib.mae_engine_features_workspace_bytes(mae.engine.handle, B, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    for pool in ("cls", "mean"):
        for norm in ("none", "l2"):
            want = mae.extract_features(imgs, pool=pool, normalize=norm)
            buf = torch.full((B * D + 8,), float("nan"), device=dev)
            assert buf.data_ptr() % 16 == 0
            check(lib.mae_engine_extract_features(mae.engine.handle, _ptr(mae.flat_params), _ptr(mae._weights()), _ptr(imgs), mae._img_dt(imgs), B, 1,
                                                  FEATURE_POOLS[pool], FEATURE_NORMS[norm], _ptr(ws), need, _ptr(buf[1:]), _stream(dev)))
            torch.cuda.synchronize()
            got = buf[1:1 + B * D].view(B, D)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (pool, norm)
            assert torch.isnan(buf[:1]).all() and torch.isnan(buf[1 + B * D:]).all(), (pool, norm)


def test_classifier_rejects_mean_patches_pool(dev):
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    mae, _ = build_mae(dev, "fp32")
    B, C = 2, 10
    n = lib.mae_engine_classifier_workspace_bytes(mae.engine.handle, B, C)
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    head = torch.zeros(C * MICRO.embed_dim + C, device=dev)
    imgs = images_of(MICRO, B, False).to(dev)
    rc = lib.mae_engine_classifier_forward(mae.engine.handle, _ptr(mae.flat_params), _ptr(mae._weights()), _ptr(head), _ptr(imgs), _lib.MAE_F32,
                                           None, B, _lib.POOL_MEAN_PATCHES, C, _ptr(ws), n, None, None, None, _stream(dev))
    assert rc != 0 and b"pool" in lib.mae_last_error()


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 5e-3)])
def test_ijepa_target_and_context_features(dev, precision, tol):
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    cfg, B = J.JEPA_MICRO, 4
    mc = dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
              encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
              predictor=dict(pred_embed_dim=cfg.pred_embed_dim, pred_depth=cfg.pred_depth, pred_num_heads=cfg.pred_num_heads))
    module = IJEPAPretrainModule(mc, dict(total_epochs=10, warmup_epochs=1, steps_per_epoch=4, batch_size=512, ema_start=0.5, ema_end=1.0))
    params = J.init_params(cfg, 73)
    J.M.randomize_params(params)
    module.model.net.load_state_dict(params)
    module.model.reset_target()
    module = module.to(dev)
    for step in (1, 2):
        images = J.M.synthetic_images(B, cfg.as_mae(), seed=100 + step)
        ctx, tgt = J.sample_masks(cfg, B, torch.Generator().manual_seed(step))
        module.fused_training_step(images.to(dev), ctx, tgt, lr=1e-2)
    model = module.model
    imgs = J.M.synthetic_images(6, cfg.as_mae(), seed=9)
    t = model.extract_features(imgs.to(dev), encoder="target").double().cpu()
    c = model.extract_features(imgs.to(dev), encoder="context").double().cpu()
    assert not torch.equal(t, c)
    ctx_p = {k: v.detach().cpu() for k, v in model.net.state_dict().items()}
    tgt_p = dict(ctx_p, **{k: v.detach().cpu() for k, v in model.target_state_dict().items()})
    patches = torch.arange(1, cfg.num_patches + 1).repeat(imgs.shape[0], 1)
    for got, p in ((t, tgt_p), (c, ctx_p)):
        with torch.no_grad():
            ref = J.encode_tokens(p, cfg, imgs, patches, bf16=precision == "bf16").double().mean(1)
        assert float((got - ref).norm() / ref.norm()) <= tol
        # bf16 per element: 3 units of 2^-8, as in test_extraction_matches_oracle
        assert float((got - ref).abs().max()) <= (tol if precision == "fp32" else 3 * 2.0 ** -8) * float(ref.abs().max())
    l2 = model.extract_features(imgs.to(dev), encoder="target", normalize="l2").double().cpu()
    assert torch.allclose(l2, t / (t.norm(dim=1, keepdim=True) + 1e-8), rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError):
        model.extract_features(imgs.to(dev), pool="cls")


def test_vits8_b2000_bf16(dev):
    cfg = O.MAEConfig(image_size=96, patch_size=8, in_chans=3, embed_dim=384, depth=12, num_heads=6,
                      decoder_embed_dim=192, decoder_depth=1, decoder_num_heads=6)
    mae, _ = build_mae(dev, "bf16", cfg)
    imgs = images_of(cfg, 2000, True, seed=3).to(dev)
    for pool in ("cls", "mean"):
        a = mae.extract_features(imgs, pool=pool)
        b = mae.extract_features(imgs, pool=pool)
        assert torch.isfinite(a).all() and torch.equal(a, b)
        parts = torch.cat([mae.extract_features(imgs[i:i + 500], pool=pool) for i in range(0, 2000, 500)])
        assert float((parts - a).abs().max()) <= 1e-5 * float(a.abs().max()), pool


# ------------------------------------------------------------------------------------------------------------------
# k-NN
# ------------------------------------------------------------------------------------------------------------------
def _rows(n, d, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(dev)


@pytest.mark.parametrize("Q,N,D,k", [(1, 1, 4, 1), (777, 5003, 144, 20), (777, 5003, 384, 256), (8000, 5000, 384, 200), (64, 100_000, 384, 20),
                                     (33, 300, 12, 7)])
def test_topk_matches_fp64(dev, Q, N, D, k):
    from ssrl_vit_mae_jepa_amd.representation import knn_topk
    q, b = _rows(Q, D, 1, dev), _rows(N, D, 2, dev)
    sims, idx = knn_topk(q, b, k)
    ref, bound = topk_ref(q, b)
    check_topk(sims, idx, ref, bound, k)
    s2, i2 = knn_topk(q, b, k)
    assert torch.equal(sims, s2) and torch.equal(idx, i2)


def test_topk_ties_nan_and_k_equal_n(dev):
    from ssrl_vit_mae_jepa_amd.representation import knn_topk
    b = _rows(40, 16, 3, dev)
    b[25] = b[7]                                # duplicated rows: the lower index comes first
    b[31] = float("nan")                        # a NaN row never comes ahead of a finite one
    q = torch.cat([b[7:8], _rows(5, 16, 4, dev)])
    sims, idx = knn_topk(q, b, 40)
    i0 = idx[0].tolist()
    assert i0[0] == 7 and i0[1] == 25 and sims[0, 0] == sims[0, 1]
    for r in range(q.shape[0]):
        row = idx[r].tolist()
        assert sorted(row) == list(range(40))  # k = N returns every row once
        assert row[-1] == 31 and sims[r, -1] == float("-inf")
        assert torch.isfinite(sims[r, :-1]).all()


def test_topk_split_invariance(dev):
    from ssrl_vit_mae_jepa_amd.representation import knn_topk
    q, b = _rows(500, 384, 5, dev), _rows(20_000, 384, 6, dev)
    sims, idx = knn_topk(q, b, 50)
    sub = torch.arange(3, 500, 7, device=dev)
    s_sub, i_sub = knn_topk(q[sub].contiguous(), b, 50)         # a query subset: other Q, query tiles and bank splits
    assert torch.equal(s_sub, sims[sub]) and torch.equal(i_sub, idx[sub])
    s_pre, i_pre = knn_topk(q, b[:1234].contiguous(), 256)      # a bank prefix: every pair seen twice has the same bits
    shared = 0
    for r in range(500):
        m = dict(zip(i_pre[r].tolist(), s_pre[r].tolist()))
        for s, i in zip(sims[r].tolist(), idx[r].tolist()):
            if i in m:
                assert s == m[i], (r, i)
                shared += 1
    assert shared > 500


def test_vote_matches_fp64(dev):
    from ssrl_vit_mae_jepa_amd.representation import knn_topk, knn_vote
    Q, N, C, T = 300, 2000, 10, 0.07
    q = torch.nn.functional.normalize(_rows(Q, 64, 7, dev), dim=1)
    b = torch.nn.functional.normalize(_rows(N, 64, 8, dev), dim=1)
    labels = torch.randint(0, C, (N,), generator=torch.Generator().manual_seed(9)).to(dev)
    sims, idx = knn_topk(q, b, 200)
    for k in (1, 10, 20, 100, 200):
        scores, pred = knn_vote(sims, idx, labels, C, k=k, temperature=T, return_scores=True)
        rs, rp = vote_ref(sims, idx, labels, C, k, T)
        assert torch.allclose(scores.double().cpu(), rs, rtol=1e-5, atol=0)
        assert torch.equal(pred.cpu(), rp) or (pred.cpu() != rp).sum() <= 1
    # ties go to the lowest class; k < k_stride reads the first k columns only
    s = torch.tensor([[0.5, 0.5, 0.1], [0.3, 0.2, 0.9]], device=dev)
    i = torch.tensor([[0, 1, 2], [2, 0, 1]], device=dev)
    lab = torch.tensor([3, 1, 0], device=dev)
    assert knn_vote(s, i, lab, 4, k=2).tolist() == [1, 0]
    assert knn_vote(s, i, lab, 4, k=3).tolist() == [1, 1]
    scores, pred = knn_vote(s, i, torch.tensor([3, 7, 0], device=dev), 4, k=2, return_scores=True)
    assert pred.tolist() == [-1, 0] and torch.isnan(scores[0]).all() and torch.isfinite(scores[1]).all()
    scores, pred = knn_vote(s[:1], i[:1], torch.tensor([3, 1, 9], device=dev), 4, k=2, return_scores=True)
    assert pred.tolist() == [1] and torch.isfinite(scores).all()


def test_self_retrieval(dev):
    from ssrl_vit_mae_jepa_amd.representation import knn_classify, knn_topk
    mae, _ = build_mae(dev, "fp32")
    imgs = images_of(MICRO, 300, True, seed=12).to(dev)
    f = mae.extract_features(imgs, pool="cls", normalize="l2")
    sims, idx = knn_topk(f, f, 5)
    assert torch.equal(idx[:, 0].cpu(), torch.arange(300))
    labels = torch.arange(300, device=dev) % 10
    assert knn_classify(f, labels, f, labels, ks=[1], num_classes=10)[1] == 1.0


# ------------------------------------------------------------------------------------------------------------------
# CLI
# ------------------------------------------------------------------------------------------------------------------
def test_knn_eval_cli(dev, tmp_path):
    import yaml
    from ssrl_vit_mae_jepa_amd.data import get_test_batches, synthetic_labeled
    from ssrl_vit_mae_jepa_amd.representation import extract_split_features, knn_classify, load_eval_encoder
    from ssrl_vit_mae_jepa_amd.data import LabeledBatches
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True, timeout=600)  # noqa: E731
    mae_cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    mae_cfg["logging"]["output_dir_base"] = str(tmp_path / "mae")
    mae_cfg["pretrain"]["batch_size"] = 256
    ij_cfg = yaml.safe_load((ROOT / "configs" / "ijepa_vits8.yaml").read_text())
    ij_cfg["logging"]["output_dir_base"] = str(tmp_path / "ij")
    ij_cfg["model"]["encoder"] = dict(embed_dim=144, depth=2, num_heads=6)
    ij_cfg["model"]["predictor"] = dict(pred_embed_dim=96, pred_depth=1, pred_num_heads=6)
    ij_cfg["pretrain"]["batch_size"] = 128
    ij_cfg["pretrain"]["total_epochs"] = 1
    paths = {}
    for name, cfg in (("mae", mae_cfg), ("ij", ij_cfg)):
        paths[name] = tmp_path / f"{name}.yaml"
        paths[name].write_text(yaml.safe_dump(cfg))
    r = run("scripts.training.pretrain_mae", "--config", str(paths["mae"]), "--synthetic_images", "256", "--max_epochs", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    r = run("scripts.training.pretrain_ijepa", "--config", str(paths["ij"]), "--synthetic_images", "256", "--max_epochs", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    mae_ck = tmp_path / "mae" / "pretrain" / "mae_pretrain" / "checkpoints" / "last.ckpt"
    ij_ck = tmp_path / "ij" / "pretrain" / "ijepa_pretrain" / "checkpoints" / "last.ckpt"
    n_syn = 500
    cases = [("mae", mae_ck, "target"), ("mae", "random", "target"), ("ij", ij_ck, "target"), ("ij", ij_ck, "context")]
    for name, ck, which in cases:
        out = tmp_path / f"out_{name}_{which}_{Path(str(ck)).name}"
        r = run("scripts.evaluation.knn_eval", "--config", str(paths[name]), "--checkpoint", str(ck), "--encoder", which, "--k", "10,20",
                "--synthetic_images", str(n_syn), "--batch_size", "128", "--output_dir", str(out), "--save_features")
        assert r.returncode == 0, r.stderr[-3000:]
        res = json.loads(r.stdout.strip().splitlines()[-1])
        assert json.loads((out / "knn.json").read_text()) == res
        assert res["bank_size"] == n_syn and set(res["top1"]) == {"10", "20"}
        # the same numbers from an in-process run on the same features
        feats = torch.load(out / "knn_features.pt", map_location="cpu", weights_only=True)
        acc = knn_classify(feats["bank"].to(dev), feats["bank_labels"].to(dev), feats["queries"].to(dev), feats["query_labels"].to(dev),
                           ks=[10, 20], num_classes=10)
        assert {str(k): v for k, v in acc.items()} == res["top1"], (name, which)
        assert res["kind"] == ("random" if ck == "random" else ("ijepa" if name == "ij" else "mae"))
    r = run("scripts.evaluation.knn_eval", "--config", str(paths["ij"]), "--checkpoint", str(ij_ck), "--pool", "cls",
            "--synthetic_images", str(n_syn), "--output_dir", str(tmp_path / "bad"))
    assert r.returncode != 0


def test_visualize_representation_tsne(dev, tmp_path):
    pytest.importorskip("sklearn")
    pytest.importorskip("matplotlib")
    import numpy as np
    run = subprocess.run([sys.executable, "-m", "scripts.evaluation.visualize_representation", "--config", str(ROOT / "configs" / "mae.yaml"),
                          "--encoder_ckpt", "random", "--method", "tsne", "--pool", "mean", "--normalize", "channel", "--max_samples", "200",
                          "--batch_size", "64", "--synthetic_images", "200", "--output_dir", str(tmp_path), "--save_features"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-3000:]
    stem = "representation_random_tsne_mean_channel"
    pngs = sorted(p.name for p in tmp_path.glob("*.png"))
    assert f"{stem}.png" in pngs and len(pngs) == 11, pngs
    z = np.load(tmp_path / f"{stem}.npz")
    assert z["features"].shape == (200, 144) and z["labels"].shape == (200,) and z["projection"].shape == (200, 2)
    np.testing.assert_allclose(z["features"].mean(0), 0, atol=1e-5)  # channel-normalised on the host
