"""Host-side checks of the linear probe (no GPU): the fp64 reference of tests/probe_ref.py against torch, the fold, the geometry the
bounds count with, that the BatchNorm test data tells a one-sweep variance from a centred one, config parsing, the pool-name map, the
checkpoint's keys and the CLI's argument errors."""
import math
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from oracle import mae_oracle as O
from tests import probe_ref as R

ROOT = Path(__file__).resolve().parents[1]
CFG = str(ROOT / "configs" / "vits8_dec192_linprobe.yaml")
MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


def model_cfg(cfg=MICRO, pool="cls"):
    return dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision="fp32"),
                encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                decoder=dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads),
                head=dict(embed_dim=cfg.embed_dim, pool=pool))


def rel(a, b) -> float:
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- the reference against torch ----------------------------------------------------------------------------------------
def test_bn_reference_matches_torch_batchnorm():
    D = 24
    bn = torch.nn.BatchNorm1d(D, affine=False, eps=R.f32(1e-6), momentum=R.f32(0.1)).double()
    rm, rv = np.zeros(D), np.ones(D)
    r = np.random.default_rng(3)
    bn.train()
    for rows in (7, 2, 33):
        x = (r.standard_normal((rows, D)) * r.uniform(0.05, 4.0, D) + r.uniform(-8, 8, D)).astype(np.float32)
        want = bn(torch.from_numpy(x).double()).numpy()
        ref = R.bn_train(x, rm, rv, 1e-6, 0.1)
        rm, rv = ref["running_mean"], ref["running_var"]
        assert rel(ref["y"], want) < 1e-12
        assert rel(rm, bn.running_mean.numpy()) < 1e-12 and rel(rv, bn.running_var.numpy()) < 1e-12
    untracked = R.bn_train(x, None, None, 1e-6, 0.1)
    assert untracked["running_mean"] is None and np.array_equal(untracked["y"], ref["y"])
    bn.eval()
    x = r.standard_normal((5, D)).astype(np.float32)
    assert rel(R.bn_eval(x, rm, rv, 1e-6)["y"], bn(torch.from_numpy(x).double()).numpy()) < 1e-12
    assert int(bn.num_batches_tracked) == 3


def torch_lars(p, g, mu, adapt, lr, momentum, weight_decay, trust_coefficient):
    """The definition, literally, in fp64 torch: the LARS of the MAE code base with `adapt` for p.ndim > 1."""
    p, g, mu = (torch.from_numpy(np.asarray(t, dtype=np.float64)).clone() for t in (p, g, mu))
    lr, momentum, weight_decay, trust_coefficient = (R.f32(v) for v in (lr, momentum, weight_decay, trust_coefficient))
    dp = g
    if adapt:
        dp = dp.add(p, alpha=weight_decay)
        param_norm, update_norm = torch.norm(p), torch.norm(dp)
        one = torch.ones_like(param_norm)
        q = torch.where(param_norm > 0.0, torch.where(update_norm > 0, trust_coefficient * param_norm / update_norm, one), one)
        dp = dp.mul(q)
    mu = mu.mul(momentum).add(dp)
    p = p.add(mu, alpha=-lr)
    return p.numpy(), mu.numpy()


@pytest.mark.parametrize("name,wd,zero_p,zero_g", [("plain", 0.0, False, False), ("decay", 0.05, False, False), ("zero_p", 0.05, True, False),
                                                   ("zero_g", 0.0, False, True)])
@pytest.mark.parametrize("adapt", [1, 0])
def test_lars_reference_matches_the_definition(name, wd, zero_p, zero_g, adapt):
    n = 96
    p, g, mu = R.gen_lars(n, 5, zero_p=zero_p, zero_g=zero_g, zero_mu=True)
    tp, tmu = p.astype(np.float64), mu.astype(np.float64)
    rp, rmu = tp.copy(), tmu.copy()
    for step in range(3):
        gs = g if zero_g else R.gen_lars(n, 6 + step)[1]
        tp, tmu = torch_lars(tp, gs, tmu, adapt, 0.78, 0.9, wd, 0.001)
        ref = R.lars_step(rp, gs, rmu, adapt, 0.78, 0.9, wd, 0.001)
        if step == 0 and adapt and (zero_p or zero_g):
            assert ref["q"] == 1.0   # a zero norm: no trust ratio
        elif step == 0 and adapt:
            assert ref["q"] != 1.0
        rp, rmu = ref["p"], ref["mu"]
        assert rel(rp, tp) < 1e-12 and np.abs(rmu - tmu).max() <= 1e-12 * max(np.abs(tmu).max(), 1e-300)


def test_fold_equals_bn_eval_then_linear():
    from ssrl_vit_mae_jepa_amd.probe import fold
    r = np.random.default_rng(11)
    B, D, C = 9, 20, 7
    x = (r.standard_normal((B, D)) * 3 + 5).astype(np.float32)
    w, b = (0.01 * r.standard_normal((C, D))).astype(np.float32), r.standard_normal(C).astype(np.float32)
    rm, rv = R.gen_running(D)
    want = R.head(R.bn_eval(x, rm, rv, 1e-6)["y"], w, b)["logits"]
    for f in (R.fold, fold):
        wf, bf = f(w, b, rm, rv, 1e-6)
        assert rel(x.astype(np.float64) @ wf.T + bf, want) < 1e-12


def test_probe_step_reference_is_its_pieces():
    r = np.random.default_rng(2)
    B, D, C = 6, 8, 3
    x, lab = r.standard_normal((B, D)).astype(np.float32), r.integers(0, C, B)
    w, b = (0.01 * r.standard_normal((C, D))).astype(np.float32), np.zeros(C, np.float32)
    cfg = dict(bn_eps=1e-6, bn_momentum=0.1, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001)
    out = R.probe_step(w, b, np.zeros(C * D), np.zeros(C), np.zeros(D), np.ones(D), x, lab, 0.5, cfg)
    y = torch.from_numpy(out["bn"]["y"]).requires_grad_(False)
    W, bb = torch.from_numpy(w.astype(np.float64)).requires_grad_(), torch.from_numpy(b.astype(np.float64)).requires_grad_()
    loss = torch.nn.functional.cross_entropy(y @ W.T + bb, torch.from_numpy(lab))
    loss.backward()
    assert abs(float(loss.detach()) - out["head"]["loss"]) < 1e-12
    assert rel(out["head"]["dW"], W.grad.numpy()) < 1e-12 and rel(out["head"]["db"], bb.grad.numpy()) < 1e-12
    assert out["lars_b"]["q"] == 1.0 and np.array_equal(out["lars_b"]["d"], out["head"]["db"])


# ---- geometry and data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,dim", R.BN_SHAPES + [(2000, 384), (16384, 1024), (5, 4), (70000, 8), (1 << 20, 1024)])
def test_geometry_matches_the_library(rows, dim):
    from ssrl_vit_mae_jepa_amd._lib import lib
    g = R.bn_geometry(rows, dim)
    assert lib.mae_batchnorm_scratch_bytes(rows, dim) == g["scratch_bytes"]
    assert g["grid"] <= R.BN_MAX_BLOCKS and g["slice"] % g["rp"] == 0 and g["grid"] * g["slice"] >= rows > (g["grid"] - 1) * g["slice"]
    assert g["rp"] * g["d4"] <= 256


def test_scratch_bytes_refuses_bad_shapes():
    from ssrl_vit_mae_jepa_amd._lib import lib
    for rows, dim in ((8, 6), (8, 1028), (8, 0), (0, 8), ((1 << 40) // 8, 8)):
        assert lib.mae_batchnorm_scratch_bytes(rows, dim) == -1


@pytest.mark.parametrize("rows,dim", R.BN_SHAPES)
def test_data_tells_one_sweep_from_centred(rows, dim):
    """A y formed with the fp32 one-sweep variance E[x^2] - E[x]^2 leaves the bound on this data at every shape; the same formula with the
    float64 variance rounded to fp32 stays inside."""
    x = R.gen_bn(rows, dim)
    ref = R.bn_train(x)
    b = R.bn_train_bounds(ref, rows, dim)
    mean32 = ref["mean"].astype(np.float32)

    def y_with(var32):
        rstd = (1.0 / np.sqrt(var32.astype(np.float64) + R.f32(1e-6))).astype(np.float32)
        return (x - mean32) * rstd

    naive = np.maximum(R.one_sweep_var_fp32(x), 0.0)
    bad, _ = R.worst(y_with(naive), ref["y"], b["y"])
    good, _ = R.worst(y_with(ref["var"].astype(np.float32)), ref["y"], b["y"])
    print(f"{rows}x{dim}: one-sweep y error / bound {bad:.3g}, centred {good:.3g}")
    assert good <= 1.0
    assert bad > 4.0
    c = R.const_column(dim)
    assert ref["var"][c] == 0.0 and np.all(ref["y"][:, c] == 0.0)


def test_exact_data_is_exact():
    x = R.gen_bn_exact(256, 148)
    ref = R.bn_train(x)
    assert np.array_equal(ref["mean"].astype(np.float32).astype(np.float64), ref["mean"])   # representable: the kernel must hit it


def test_lars_bounds_are_small_and_finite():
    for n in (4, 1440, R.LARS_WRAP + 1024):
        p, g, mu = R.gen_lars(n, 1)
        ref = R.lars_step(p, g, mu, 1, 0.78, 0.9, 0.05, 0.001)
        b = R.lars_bounds(ref, n)
        assert np.all(np.isfinite(b["p"])) and np.all(b["p"] <= 1e-5 * (np.abs(ref["p"]) + 1e-3))
    assert R.sumsq_chain(R.LARS_WRAP + 1024) == R.sumsq_chain(R.LARS_WRAP) + 1   # the count past one grid pass adds a trip


# ---- config, pools, checkpoint ------------------------------------------------------------------------------------------
def test_probe_config_defaults_and_errors():
    from ssrl_vit_mae_jepa_amd.probe import PROBE_DEFAULTS, parse_probe, probe_lr
    cfg = parse_probe(None)
    assert cfg == PROBE_DEFAULTS == dict(total_epochs=90, warmup_epochs=10, batch_size=2000, base_learning_rate=0.1, weight_decay=0.0, momentum=0.9,
                                         trust_coefficient=0.001, bn_eps=1e-6, bn_momentum=0.1, head_init_std=0.01, augment="none")
    assert probe_lr(cfg) == 0.1 * 2000 / 256
    assert probe_lr(parse_probe(dict(batch_size=512, base_learning_rate=0.2))) == 0.2 * 512 / 256
    with pytest.raises(ValueError, match="learning_rat"):
        parse_probe(dict(learning_rat=0.1))
    with pytest.raises(ValueError, match="augment"):
        parse_probe(dict(augment="randaugment"))
    with pytest.raises(ValueError, match="batch_size"):
        parse_probe(dict(batch_size=1))
    shipped = yaml.safe_load(open(CFG))
    assert parse_probe(shipped["probe"]) == PROBE_DEFAULTS


def test_cli_flags_override_the_yaml():
    from scripts.evaluation import linear_probe as L
    args = L.parse_args(["--checkpoint", "random", "--batch_size", "32", "--augment", "crop", "--base_learning_rate", "0.2"])
    cfg = L.probe_config(dict(probe=dict(batch_size=64, momentum=0.8)), args)
    assert (cfg["batch_size"], cfg["augment"], cfg["base_learning_rate"], cfg["momentum"], cfg["total_epochs"]) == (32, "crop", 0.2, 0.8, 90)
    assert args.output_dir_suffix == "linprobe" and args.encoder == "target" and args.pool is None and args.max_epochs is None


def test_epoch_batches_shuffle_and_drop_a_single_row():
    from scripts.evaluation.linear_probe import epoch_batches
    a, b, again = epoch_batches(65, 32, 73, 0), epoch_batches(65, 32, 73, 1), epoch_batches(65, 32, 73, 0)
    assert [len(x) for x in a] == [32, 32]                       # the 65th row alone cannot be normalised
    assert [len(x) for x in epoch_batches(66, 32, 73, 0)] == [32, 32, 2]
    assert all(np.array_equal(x, y) for x, y in zip(a, again)) and not np.array_equal(a[0], b[0])
    assert sorted(np.concatenate(epoch_batches(66, 32, 73, 5)).tolist()) == list(range(66))


def test_pool_names():
    from ssrl_vit_mae_jepa_amd.classifier import NO_CLS_POOL, POOLS
    from ssrl_vit_mae_jepa_amd.mae import FEATURE_POOLS
    from ssrl_vit_mae_jepa_amd.probe import CLASSIFIER_POOL, classifier_pool
    assert CLASSIFIER_POOL == {"cls": "cls", "mean": "mean_patches", "mean_all": "mean"}
    for feature, classifier in CLASSIFIER_POOL.items():
        assert FEATURE_POOLS[feature] == POOLS[classifier]            # both names mean the same pool of the C ABI
        assert classifier_pool(feature, True) == classifier
    assert classifier_pool("mean", False) == "mean_patches" and classifier_pool("mean_all", False) == "mean"
    with pytest.raises(ValueError) as e:
        classifier_pool("cls", False)
    assert str(e.value) == NO_CLS_POOL
    with pytest.raises(ValueError, match="pool"):
        classifier_pool("mean_patches", True)


@pytest.mark.parametrize("pool,with_cls", [("cls", True), ("mean", True), ("mean", False)])
def test_checkpoint_keys_and_hyper_parameters(pool, with_cls, tmp_path):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, checkpoint_with_cls, encoder_mae
    from ssrl_vit_mae_jepa_amd.probe import CLASSIFIER_POOL, LinearProbe
    mc = model_cfg()
    vit = encoder_mae(mc).encoder.vit
    vit.with_cls = with_cls
    probe = LinearProbe(MICRO.embed_dim, 10, dict(head_init_std=0.02))
    head = probe.head
    assert set(head.state_dict()) == {"bn.running_mean", "bn.running_var", "bn.num_batches_tracked", "classification.classification.weight",
                                      "classification.classification.bias"}
    w = head.classification.classification.weight
    assert float(head.classification.classification.bias.detach().abs().max()) == 0.0 and 0.01 < float(w.detach().std()) < 0.03
    assert w.data_ptr() == head.flat.data_ptr()                       # the flat W-then-b layout
    with torch.no_grad():
        head.bn.running_mean.copy_(torch.linspace(-1, 1, MICRO.embed_dim))
        head.bn.running_var.copy_(torch.linspace(0.5, 2, MICRO.embed_dim))
    ck = probe.classifier_checkpoint(vit, mc, pool, epoch=4)
    torch.save(ck, tmp_path / "c.ckpt")
    ck = torch.load(tmp_path / "c.ckpt", map_location="cpu", weights_only=True)     # as build_module loads it
    module = ViTClassifierTrainModule(pretrained_encoder=encoder_mae(mc).encoder.vit, model_cfg=mc, training_cfg={}, num_classes=10)
    assert set(ck["state_dict"]) == set(module.state_dict())
    hp = ck["hyper_parameters"]
    assert set(hp) == {"model_cfg", "training_cfg", "num_classes", "with_cls"}
    assert hp["with_cls"] is with_cls and checkpoint_with_cls(ck) is with_cls and hp["num_classes"] == 10
    assert hp["model_cfg"]["head"]["pool"] == CLASSIFIER_POOL[pool] and hp["model_cfg"]["encoder"] == mc["encoder"]
    assert mc["head"]["pool"] == "cls"                                # the caller's config is not edited
    wf, bf = R.fold(w.detach().numpy(), np.zeros(10), head.bn.running_mean.numpy(), head.bn.running_var.numpy(), 1e-6)
    assert np.array_equal(ck["state_dict"]["model.head.classification.weight"].numpy(), wf.astype(np.float32))
    assert np.array_equal(ck["state_dict"]["model.head.classification.bias"].numpy(), bf.astype(np.float32))
    if not with_cls:
        with pytest.raises(ValueError, match="class token"):
            probe.classifier_checkpoint(vit, mc, "cls")


def test_probe_state_round_trip():
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe
    a, b = LinearProbe(16, 5, seed=1), LinearProbe(16, 5, seed=2)
    a.mu.normal_()
    a.head.bn.running_mean.normal_()
    a.steps, a.epoch = 12, 3
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.mu, b.mu) and torch.equal(a.head.flat, b.head.flat) and torch.equal(a.head.bn.running_mean, b.head.bn.running_mean)
    assert (b.steps, b.epoch) == (12, 3)
    with pytest.raises(RuntimeError, match="MI355X"):
        a.step(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64), 0.1)   # no CPU fallback


# ---- CLI argument errors that end before any device work -------------------------------------------------------------------
def test_cli_argument_errors(tmp_path, monkeypatch):
    from scripts.evaluation import linear_probe as L
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device work was reached")))
    base = ["--config", CFG, "--checkpoint", "random"]

    def dies(argv, text):
        with pytest.raises(SystemExit) as e:
            L.main(argv)
        assert text in str(e.value), str(e.value)

    dies(base + ["--synthetic_images", "64", "--batch_size", "1"], "batch_size")
    dies(base + ["--synthetic_images", "64", "--max_epochs", "0"], "--max_epochs")
    dies(["--config", CFG, "--checkpoint", str(tmp_path / "none.ckpt"), "--synthetic_images", "64"], "not found")
    dies(base + ["--synthetic_images", "64", "--resume", str(tmp_path / "none.pt")], "--resume")
    dies(["--config", str(ROOT / "configs" / "ijepa_vits8.yaml"), "--checkpoint", "random", "--pool", "cls", "--synthetic_images", "64"], "class token")
    monkeypatch.setattr(L, "STL10_DIR", tmp_path)
    dies(base, "--synthetic_images")
    bad = yaml.safe_load(open(CFG))
    bad["probe"]["lars_eta"] = 0.001
    (tmp_path / "bad.yaml").write_text(yaml.safe_dump(bad))
    dies(["--config", str(tmp_path / "bad.yaml"), "--checkpoint", "random", "--synthetic_images", "64"], "lars_eta")
    with pytest.raises(SystemExit):
        L.parse_args(base + ["--augment", "randaugment"])
    assert math.isclose(L.probe_config({}, L.parse_args(base))["bn_eps"], 1e-6)
