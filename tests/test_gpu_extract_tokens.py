"""mae_engine_extract_tokens on the MI355X against the oracle's token output: [cls | patches] and the patches alone, the class row kept
and dropped, the I-JEPA target and context arenas, both precisions; and against mae_engine_extract_features, whose patch-row mean the
mean over the new output's patch rows must reproduce."""
import numpy as np
import pytest
import torch

from oracle import jepa_oracle as J
from oracle import mae_oracle as O

pytestmark = pytest.mark.gpu

MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)
U = 2.0 ** -24


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


def images_of(cfg, B, seed=11):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, cfg.in_chans, cfg.image_size, cfg.image_size), dtype=torch.uint8, generator=g)
    return (x.float() / 255 - 0.5) / 0.5


def relnorm(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# the tolerances of tests/test_gpu_representation.py::test_extraction_matches_oracle for pooled features, as relative norms
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_tokens_match_the_oracle(dev, precision, tol):
    mae, params = build_mae(dev, precision)
    B, L, D = 9, MICRO.sequence_length, MICRO.embed_dim
    imgs = images_of(MICRO, B)
    bf = precision == "bf16"
    with torch.no_grad():
        ref_cls = O.forward_encoder(params, MICRO, imgs, bf16=bf)                                 # (B, L, D): [cls | patches]
        ref_nocls = O.forward_encoder(params, MICRO, imgs, idx_keep=torch.arange(1, L).repeat(B, 1), bf16=bf)
    x = imgs.to(dev)
    kept = mae.extract_tokens(x, with_cls=True, drop_cls=False)
    dropped = mae.extract_tokens(x, with_cls=True, drop_cls=True)
    alone = mae.extract_tokens(x, with_cls=False)
    assert kept.shape == (B, L, D) and dropped.shape == (B, L - 1, D) and alone.shape == (B, L - 1, D)
    assert kept.dtype == torch.float32 and not kept.requires_grad
    for name, got, ref in (("kept", kept, ref_cls), ("dropped", dropped, ref_cls[:, 1:]), ("alone", alone, ref_nocls)):
        r = relnorm(got.cpu(), ref)
        print(f"{precision} {name}: relative norm {r:.3g}")
        assert r <= tol, (name, r)
    assert torch.equal(dropped, kept[:, 1:])                                                       # the same rows, the same bits
    assert torch.equal(kept, mae.extract_tokens(x, with_cls=True, drop_cls=False))                 # deterministic
    assert torch.equal(mae.encoder.vit.extract_tokens(x), dropped)
    u8 = torch.randint(0, 256, (B, 3, MICRO.image_size, MICRO.image_size), dtype=torch.uint8, generator=torch.Generator().manual_seed(11))
    assert torch.equal(mae.extract_tokens(u8.to(dev), with_cls=True, drop_cls=False), kept)        # raw pixels: the same tokens


def test_patch_row_mean_is_the_pooled_feature(dev):
    """fp32: the fp64 mean over the patch rows of the new output against MAE_POOL_MEAN_PATCHES of mae_engine_extract_features.  Both
    kernels evaluate the same LayerNorm of the same fp32 rows, each in fp32 with its own summation order, and the pool then adds T
    terms and divides.  Per element, with A = mean_t |y|: the T-term mean (T + 1) u A; the two LayerNorm evaluations differ by at most
    K = 60 roundings (twice a 22-long sum chain and 8 more operations) on |y - beta| and, through the row mean, on |gamma| rho, where
    rho = mean|x| rstd <= sqrt(1 + (m / sigma)^2) < 4 for a row whose mean lies within 3 standard deviations of zero."""
    mae, params = build_mae(dev, "fp32")
    B = 9
    x = images_of(MICRO, B).to(dev)
    gamma = params["encoder.vit.norm.weight"].double().abs()
    beta = params["encoder.vit.norm.bias"].double()
    for with_cls in (True, False):
        toks = mae.extract_tokens(x, with_cls=with_cls, drop_cls=True).double().cpu()
        feats = mae.extract_features(x, pool="mean", normalize="none", with_cls=with_cls).double().cpu()
        T = toks.shape[1]
        bound = U * ((T + 1) * toks.abs().mean(1) + 60.0 * ((toks - beta).abs().mean(1) + 4.0 * gamma))
        ratio = float(((toks.mean(1) - feats).abs() / bound).max())
        print(f"with_cls {with_cls}: worst |mean of tokens - pooled feature| / bound {ratio:.3g}")
        assert ratio <= 1.0


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_ijepa_target_and_context_tokens(dev, precision, tol):
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    from ssrl_vit_mae_jepa_amd.representation import EvalEncoder
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
    for step in (1, 2):   # two steps: the EMA target arena leaves the context encoder
        images = J.M.synthetic_images(B, cfg.as_mae(), seed=100 + step)
        ctx, tgt = J.sample_masks(cfg, B, torch.Generator().manual_seed(step))
        module.fused_training_step(images.to(dev), ctx, tgt, lr=1e-2)
    model = module.model
    imgs = J.M.synthetic_images(6, cfg.as_mae(), seed=9)
    t = model.extract_tokens(imgs.to(dev), encoder="target").cpu()
    c = model.extract_tokens(imgs.to(dev), encoder="context").cpu()
    assert t.shape == (6, cfg.num_patches, cfg.embed_dim) and not torch.equal(t, c)
    ctx_p = {k: v.detach().cpu() for k, v in model.net.state_dict().items()}
    tgt_p = dict(ctx_p, **{k: v.detach().cpu() for k, v in model.target_state_dict().items()})
    patches = torch.arange(1, cfg.num_patches + 1).repeat(imgs.shape[0], 1)
    for name, got, p in (("target", t, tgt_p), ("context", c, ctx_p)):
        with torch.no_grad():
            ref = J.encode_tokens(p, cfg, imgs, patches, bf16=precision == "bf16")
        r = relnorm(got, ref)
        print(f"{precision} I-JEPA {name}: relative norm {r:.3g}")
        assert r <= tol, (name, r)
    enc = EvalEncoder("ijepa", "ijepa_ckpt", "target", ijepa=model)
    assert torch.equal(enc.tokens(imgs.to(dev)).cpu(), t) and enc.num_heads == cfg.num_heads and not enc.with_cls
    with pytest.raises(ValueError):
        model.extract_tokens(imgs.to(dev), encoder="both")


def test_refusals(dev):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    mae, _ = build_mae(dev, "fp32")
    B = 3
    x = images_of(MICRO, B).to(dev)
    h = mae.engine.handle
    need = lib.mae_engine_tokens_workspace_bytes(h, B, 0)
    assert need == lib.mae_engine_features_workspace_bytes(h, B, 0) > 0 and lib.mae_engine_tokens_workspace_bytes(h, 0, 1) == -1
    ws = torch.empty(lib.mae_engine_tokens_workspace_bytes(h, B, 1), dtype=torch.uint8, device=dev)
    out = torch.full((B, MICRO.sequence_length, MICRO.embed_dim), float("nan"), device=dev)
    for with_cls, drop, size, word in ((0, 1, ws.numel(), "drop_cls"), (2, 0, ws.numel(), "with_cls"), (1, 2, ws.numel(), "drop_cls"), (1, 0, 256, "workspace")):
        rc = lib.mae_engine_extract_tokens(h, _ptr(mae.flat_params), _ptr(mae._weights()), _ptr(x), 0, B, with_cls, drop, _ptr(ws), size, _ptr(out), _stream(dev))
        torch.cuda.synchronize()
        assert rc != 0 and word.encode() in lib.mae_last_error(), (with_cls, drop, lib.mae_last_error())
        assert bool(torch.isnan(out).all())
