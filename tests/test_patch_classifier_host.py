"""Host-side checks (no GPU) of the classifier on patch-only encoders: the four ``_ex`` symbols, pool validation, the
``with_cls`` checkpoint key, the I-JEPA -> classifier encoder loader and the fine-tuning CLI's arguments."""
import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "mae_hip.h"
EX_SYMBOLS = ("mae_engine_classifier_workspace_bytes_ex", "mae_engine_classifier_forward_ex", "mae_engine_classifier_loss_and_grads_ex",
              "mae_classifier_head_ex")
TINY = dict(general=dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32"), encoder=dict(embed_dim=32, depth=2, num_heads=2))
IJ = dict(TINY, predictor=dict(pred_embed_dim=32, pred_depth=1, pred_num_heads=2))


def test_ex_symbols_in_header_and_binding():
    from ssrl_vit_mae_jepa_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", HEADER.read_text(), flags=re.S)
    for n in EX_SYMBOLS:
        assert re.search(rf"\b{n}\s*\(", text), n
        assert n in _lib.SIGNATURES and hasattr(_lib.lib, n)
    assert _lib.ABI_VERSION == 4
    # one more int32 (with_cls) than the entry point each one extends
    for n in EX_SYMBOLS:
        assert len(_lib.SIGNATURES[n][1]) == len(_lib.SIGNATURES[n[:-3]][1]) + 1


def test_ex_workspace_metadata():
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd.mae import Engine
    e = Engine(dict(image_size=96, patch_size=8, in_chans=3, embed_dim=384, depth=12, num_heads=6, decoder_embed_dim=384,
                    decoder_depth=1, decoder_num_heads=6), "bf16")
    f, h = _lib.lib.mae_engine_classifier_workspace_bytes_ex, e.handle
    assert f(h, 64, 10, 1) == _lib.lib.mae_engine_classifier_workspace_bytes(h, 64, 10)
    assert 0 < f(h, 64, 10, 0) < f(h, 64, 10, 1)  # 144 rows instead of 145 and no decoder-sized buffers
    for bad in ((0, 10, 0), (64, 1, 0), (64, 129, 1), (64, 10, 2), (64, 10, -1)):
        assert f(h, *bad) == -1, bad
    assert f(None, 64, 10, 0) == -1


def _vit(with_cls=True):
    from ssrl_vit_mae_jepa_amd.classifier import encoder_mae
    vit = encoder_mae(TINY).encoder.vit
    vit.with_cls = with_cls
    return vit


def test_pool_validation():
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifier
    assert _vit().with_cls is True  # the node's default
    for with_cls in (True, False):
        for pool in ("mean", "mean_patches"):
            clf = ViTClassifier(_vit(with_cls), 10, {"pool": pool})
            assert (clf.pool_type, clf.with_cls) == (pool, with_cls)
            assert clf.extended == (not with_cls or pool == "mean_patches")
    assert not ViTClassifier(_vit(), 10, {"pool": "cls"}).extended and not ViTClassifier(_vit(), 10).extended
    with pytest.raises(ValueError, match="class token"):
        ViTClassifier(_vit(False), 10, {"pool": "cls"})
    with pytest.raises(ValueError, match="class token"):
        ViTClassifier(_vit(False), 10)  # the default pool is cls
    with pytest.raises(ValueError, match="mean_patches"):
        ViTClassifier(_vit(), 10, {"pool": "max"})


def _module(with_cls, pool):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule
    mc = dict(TINY, head=dict(embed_dim=32, pool=pool))
    return ViTClassifierTrainModule(pretrained_encoder=_vit(with_cls), model_cfg=mc, training_cfg=dict(freeze_encoder=False))


def test_checkpoint_with_cls_round_trip(tmp_path):
    from scripts.training import train_mae
    from ssrl_vit_mae_jepa_amd.classifier import checkpoint_with_cls
    from ssrl_vit_mae_jepa_amd.representation import load_eval_encoder
    ck = _module(False, "mean_patches").checkpoint(1)
    assert ck["hyper_parameters"]["with_cls"] is False and checkpoint_with_cls(ck) is False
    ck_cls = _module(True, "mean").checkpoint(1)
    assert "with_cls" not in ck_cls["hyper_parameters"] and checkpoint_with_cls(ck_cls) is True  # a missing key means True
    assert checkpoint_with_cls({"state_dict": {}}) is True and checkpoint_with_cls({"hyper_parameters": {"with_cls": True}}) is True
    # the evaluation loader and the CLI's classifier branch honour the key
    enc = load_eval_encoder(ck, TINY)
    assert (enc.kind, enc.layout, enc.with_cls) == ("classifier", "classifier_ckpt", False)
    assert load_eval_encoder(ck_cls, TINY).with_cls is True
    assert load_eval_encoder(ck["state_dict"], TINY).with_cls is True  # a bare state dict carries no key
    cfg = dict(model=dict(TINY, head=dict(embed_dim=32, pool="mean")), train=dict(freeze_encoder=True))
    for c, with_cls, pool in ((ck, False, "mean_patches"), (ck_cls, True, "mean")):
        path = tmp_path / f"clf_{with_cls}.ckpt"
        torch.save(c, path)
        mod = train_mae.build_module(cfg, classifier_ckpt=str(path))
        assert (mod.model.with_cls, mod.model.pool_type) == (with_cls, pool)  # a patch-only checkpoint also carries its pool
        for k, v in c["state_dict"].items():
            assert torch.equal(mod.state_dict()[k], v), k
        assert mod.checkpoint(0)["hyper_parameters"].get("with_cls", True) == with_cls


def test_update_ranges_skip_the_unused_tensors():
    """full mode on a patch-only encoder: AdamW's arena pieces leave out exactly the cls_token slot, and pos_embed starts at row 1."""
    for with_cls in (True, False):
        mod = _module(with_cls, "mean")
        m = mod.model.mae
        lo, hi = mod._arena_range(2, 1)
        pieces, row0 = mod._update_ranges(2, 1)
        _n, c_off, c_n, _s, _f = m._offsets["encoder.vit.cls_token"]
        covered = torch.zeros(hi, dtype=torch.bool)
        for a, n in pieces:
            assert a % 4 == 0 and n % 4 == 0 and n > 0
            assert not covered[a:a + n].any()
            covered[a:a + n] = True
        if with_cls:
            assert row0 == 0 and pieces == [(lo, hi - lo)]
        else:
            assert row0 == 1 and not covered[c_off:c_off + c_n].any() and int(covered.sum()) == hi - lo - c_n
            for name, off, numel, _s, _f in m.engine.table:
                if name.startswith("encoder.vit.") and name != "encoder.vit.cls_token" and off + numel <= hi:
                    assert covered[off:off + numel].all(), name
        assert mod._update_ranges(-1, 0) == ([], 0)
        assert mod._update_ranges(1, 0)[1] == 0 and len(mod._update_ranges(1, 0)[0]) == 1


def _vit_state(seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in _vit().state_dict().items()}


def _ijepa_checkpoints(ctx, tgt):
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    pt = {**{f"encoder.vit.{k}": v for k, v in ctx.items()}, **{f"target_encoder.vit.{k}": v for k, v in tgt.items()}}
    src = IJEPAPretrainModule(IJ, {})
    with torch.no_grad():
        for name, v in src.model.net.encoder.vit.named_parameters():
            v.copy_(ctx[name])
        for name, v in src.model.target_state_dict().items():
            v.copy_(tgt[name[len("encoder.vit."):]])
    return pt, src.checkpoint_dict(0, weights_only=True)


def test_ijepa_loader_both_layouts_both_encoders():
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifier
    from ssrl_vit_mae_jepa_amd.mae import _ViT
    from ssrl_vit_mae_jepa_amd.representation import load_ijepa_encoder
    ctx, tgt = _vit_state(2), _vit_state(3)
    pt, ck = _ijepa_checkpoints(ctx, tgt)
    for src in (pt, ck, ck["state_dict"]):
        for which, ref in ((None, tgt), ("target", tgt), ("context", ctx)):
            vit = load_ijepa_encoder(src, IJ) if which is None else load_ijepa_encoder(src, IJ, encoder=which)  # target is the default
            assert isinstance(vit, _ViT) and vit.with_cls is False
            got = vit.state_dict()
            assert set(got) == set(ref)
            for k, v in ref.items():
                assert torch.equal(got[k], v), (which, k)
            assert ViTClassifier(vit, 10, {"pool": "mean_patches"}).with_cls is False
    with pytest.raises(ValueError):
        load_ijepa_encoder(pt, IJ, encoder="ema")
    # strict: a missing encoder tensor raises, in either layout
    with pytest.raises(ValueError, match="missing"):
        load_ijepa_encoder({k: v for k, v in pt.items() if "target_encoder.vit.blocks.1." not in k}, IJ)
    with pytest.raises(ValueError, match="missing"):
        load_ijepa_encoder({k: v for k, v in pt.items() if not k.startswith("encoder.vit.norm.")}, IJ, encoder="context")
    with pytest.raises(ValueError, match="predictor"):
        load_ijepa_encoder(ck, TINY)  # the arena layout of model.target_arena needs the predictor's sizes
    # an MAE checkpoint is not an I-JEPA checkpoint
    with pytest.raises(ValueError, match="I-JEPA"):
        load_ijepa_encoder({f"encoder.vit.{k}": v for k, v in ctx.items()}, IJ)


def test_train_mae_arguments_and_default_pool(tmp_path):
    from scripts.training import train_mae
    a = train_mae.parse_args([])
    assert (a.encoder, a.pool, a.encoder_ckpt, a.classifier_ckpt) == ("target", None, None, None)
    a = train_mae.parse_args(["--encoder", "context", "--pool", "mean_patches"])
    assert (a.encoder, a.pool) == ("context", "mean_patches")
    with pytest.raises(SystemExit):
        train_mae.parse_args(["--pool", "max"])
    with pytest.raises(SystemExit):
        train_mae.parse_args(["--encoder", "ema"])
    # the pool rule
    R = train_mae.resolve_pool
    assert R(dict(TINY), None, ijepa=True)["head"]["pool"] == "mean_patches"      # I-JEPA, no model.head: mean_patches
    assert R(dict(TINY, head={"pool": "mean"}), None, ijepa=True)["head"]["pool"] == "mean"
    assert R(dict(TINY, head={"pool": "mean"}), "mean_patches", ijepa=True)["head"]["pool"] == "mean_patches"  # --pool wins
    assert "pool" not in R(dict(TINY), None)["head"] and R(dict(TINY, head={"pool": "mean"}), None)["head"]["pool"] == "mean"  # MAE: unchanged
    assert R(dict(TINY), "mean_patches")["head"]["pool"] == "mean_patches"
    for mc, pool in ((dict(TINY), "cls"), (dict(TINY, head={"pool": "cls"}), None)):
        with pytest.raises(SystemExit, match="I-JEPA encoders see no class token"):
            R(mc, pool, ijepa=True)
    # build_module on an I-JEPA checkpoint of either layout, no model.head and no model.decoder in the config
    ctx, tgt = _vit_state(4), _vit_state(5)
    pt, ck = _ijepa_checkpoints(ctx, tgt)
    cfg = dict(model=IJ, train=dict(freeze_encoder=True))
    for name, obj in (("pt", pt), ("ckpt", ck)):
        path = tmp_path / f"ij.{name}"
        torch.save(obj, path)
        for which, ref in (("target", tgt), ("context", ctx)):
            mod = train_mae.build_module(cfg, encoder_ckpt=str(path), encoder=which)
            assert (mod.model.with_cls, mod.model.pool_type, mod.train_mode()) == (False, "mean_patches", (-1, 0))
            for k, v in ref.items():
                assert torch.equal(mod.model.encoder.state_dict()[k], v), (name, which, k)
        with pytest.raises(SystemExit, match="I-JEPA encoders see no class token"):
            train_mae.build_module(cfg, encoder_ckpt=str(path), pool="cls")
    # an MAE checkpoint keeps today's behaviour: --encoder is ignored, the class token stays
    mae_ck = tmp_path / "mae.ckpt"
    torch.save({"state_dict": {f"model.encoder.vit.{k}": v for k, v in ctx.items()}}, mae_ck)
    mod = train_mae.build_module(dict(model=TINY, train={}), encoder_ckpt=str(mae_ck), encoder="context")
    assert (mod.model.with_cls, mod.model.pool_type) == (True, "cls")


def test_ijepa_config_has_the_probe_sections():
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "ijepa_vits8.yaml").read_text())
    ref = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    assert cfg["model"]["head"] == {"embed_dim": 384, "pool": "mean_patches"}
    assert cfg["train"] == dict(ref["train"], freeze_encoder=True) and cfg["test"] == ref["test"]
