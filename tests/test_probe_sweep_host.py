"""Host-side checks of the linear-probe sweep (no GPU): the grid's parsing (flags over YAML, a missing axis, the refusals, parse_probe
untouched), the winner's tie-breaks, the fp64 reference's own identities, the sweep's host state and the CLI's early exit."""
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from tests import probe_ref as R
from tests import probe_sweep_ref as S

ROOT = Path(__file__).resolve().parents[1]
CFG = str(ROOT / "configs" / "vits8_dec192_linprobe.yaml")
SWEEP_CFG = str(ROOT / "configs" / "vits8_dec192_linprobe_sweep.yaml")


# ---- the grid -------------------------------------------------------------------------------------------------------------
def test_grid_parsing():
    from ssrl_vit_mae_jepa_amd.probe import PROBE_DEFAULTS, parse_probe, parse_sweep
    cfg = parse_probe(dict(base_learning_rate=0.2, weight_decay=0.001))
    assert parse_sweep(None, cfg) is None                                               # no flag, no block: no sweep
    pair = lambda lr, wd: dict(base_learning_rate=lr, weight_decay=wd)
    block = dict(base_learning_rate=[0.1, 0.3], weight_decay=[0, 0.0005])
    assert parse_sweep(block, cfg) == [pair(0.1, 0.0), pair(0.1, 0.0005), pair(0.3, 0.0), pair(0.3, 0.0005)]   # the product, lr outermost
    assert parse_sweep(block, cfg, sweep_lr="0.05, 1") == [pair(0.05, 0.0), pair(0.05, 0.0005), pair(1.0, 0.0), pair(1.0, 0.0005)]   # a flag over its key
    assert parse_sweep(block, cfg, sweep_wd="0.01") == [pair(0.1, 0.01), pair(0.3, 0.01)]
    assert parse_sweep(None, cfg, sweep_lr="0.05,0.1") == [pair(0.05, 0.001), pair(0.1, 0.001)]    # a missing axis: the single probe.* value
    assert parse_sweep(dict(weight_decay=[0.0, 0.1]), cfg) == [pair(0.2, 0.0), pair(0.2, 0.1)]
    assert parse_sweep({}, cfg) == [pair(0.2, 0.001)]                                              # an empty block: a sweep of one
    assert len(parse_sweep(None, cfg, sweep_lr=",".join(str(0.01 * (i + 1)) for i in range(8)), sweep_wd=",".join(str(0.001 * i) for i in range(8)))) == 64
    for kw, text in ((dict(sweep_lr="0.1,,0.2"), "comma-separated"), (dict(sweep_lr="0.1,x"), "no number"), (dict(sweep_lr="0.1,0"), "> 0"),
                     (dict(sweep_wd="-0.1"), ">= 0"), (dict(sweep_lr="0.1,0.1"), "repeats"), (dict(sweep_lr=""), "comma-separated"),
                     (dict(sweep_lr=",".join(str(0.01 * (i + 1)) for i in range(13)), sweep_wd="0,0.1,0.2,0.3,0.4"), "65 heads")):
        with pytest.raises(ValueError, match=text):
            parse_sweep(None, cfg, **kw)
    with pytest.raises(ValueError, match="lr"):
        parse_sweep(dict(lr=[0.1]), cfg)
    with pytest.raises(ValueError, match="mapping"):
        parse_sweep([0.1, 0.2], cfg)
    with pytest.raises(ValueError, match="empty"):
        parse_sweep(dict(base_learning_rate=[]), cfg)
    # parse_probe knows nothing of the sweep: its output is what it was, and the block sits outside probe:
    assert parse_probe(None) == PROBE_DEFAULTS and set(PROBE_DEFAULTS) == {"total_epochs", "warmup_epochs", "batch_size", "base_learning_rate", "weight_decay",
                                                                         "momentum", "trust_coefficient", "bn_eps", "bn_momentum", "head_init_std", "augment"}
    with pytest.raises(ValueError, match="probe_sweep"):
        parse_probe(dict(probe_sweep=block))
    shipped = yaml.safe_load(open(SWEEP_CFG))
    assert parse_probe(shipped["probe"]) == PROBE_DEFAULTS and shipped["probe"] == yaml.safe_load(open(CFG))["probe"]
    grid = parse_sweep(shipped["probe_sweep"], parse_probe(shipped["probe"]))
    assert len(grid) == 10 and grid[0] == pair(0.01, 0.0) and grid[-1] == pair(1.0, 0.0005)


def test_cli_grid_and_early_exit(tmp_path, monkeypatch):
    from scripts.evaluation import linear_probe as L
    from ssrl_vit_mae_jepa_amd.probe import parse_sweep
    args = L.parse_args(["--checkpoint", "random", "--sweep_lr", "0.05,0.1", "--sweep_wd", "0,0.001"])
    assert (args.sweep_lr, args.sweep_wd) == ("0.05,0.1", "0,0.001")
    none = L.parse_args(["--checkpoint", "random"])
    assert none.sweep_lr is None and none.sweep_wd is None
    assert len(parse_sweep(None, L.probe_config({}, args), args.sweep_lr, args.sweep_wd)) == 4
    # more than 64 heads: the named error, before any data is loaded or the device is asked for
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device work was reached")))
    monkeypatch.setattr(L.C, "get_train_batches", lambda *a, **k: (_ for _ in ()).throw(AssertionError("data was loaded")))
    lrs = ",".join(str(0.01 * (i + 1)) for i in range(13))
    with pytest.raises(SystemExit) as e:
        L.main(["--config", CFG, "--checkpoint", "random", "--synthetic_images", "64", "--sweep_lr", lrs, "--sweep_wd", "0,0.1,0.2,0.3,0.4"])
    assert "65 heads" in str(e.value) and "at most 64" in str(e.value)
    bad = yaml.safe_load(open(CFG))
    bad["probe_sweep"] = dict(learning_rate=[0.1])
    (tmp_path / "bad.yaml").write_text(yaml.safe_dump(bad))
    with pytest.raises(SystemExit) as e:
        L.main(["--config", str(tmp_path / "bad.yaml"), "--checkpoint", "random", "--synthetic_images", "64"])
    assert "learning_rate" in str(e.value)


# ---- the winner -----------------------------------------------------------------------------------------------------------
def test_select_tie_breaks():
    from ssrl_vit_mae_jepa_amd.probe import select
    assert select([0.1, 0.5, 0.3], [1.0, 2.0, 0.5]) == 1                 # the highest accuracy, whatever its loss
    assert select([0.5, 0.5, 0.3], [1.0, 0.9, 0.1]) == 1                 # a tie: the lower loss
    assert select([0.5, 0.5, 0.5], [0.9, 1.0, 0.9]) == 0                 # still a tie: the lower index
    assert select([0.5, 0.5], [float("nan"), 3.0]) == 1                  # a loss that is not finite loses the tie
    assert select([0.5, 0.5], [float("nan"), float("inf")]) == 0
    assert select([0.25], [1.0]) == 0
    assert select(np.array([0.1, 0.2]), torch.tensor([1.0, 1.0])) == 1
    with pytest.raises(ValueError):
        select([], [])
    with pytest.raises(ValueError):
        select([0.1], [1.0, 2.0])


# ---- the reference --------------------------------------------------------------------------------------------------------
def test_reference_of_one_head_is_probe_step():
    r = np.random.default_rng(4)
    B, D, C = 9, 12, 5
    x, lab = R.gen_bn(B, D), r.integers(0, C, B)
    W, b = S.gen_heads(1, C, D)
    mu_w, mu_b = 1e-3 * r.standard_normal(C * D), 1e-3 * r.standard_normal(C)
    rm, rv = R.gen_running(D)
    cfg = dict(bn_eps=1e-6, bn_momentum=0.1, momentum=0.9, weight_decay=0.05, trust_coefficient=0.001, batch_size=512, base_learning_rate=0.1)
    grid = [dict(base_learning_rate=0.1, weight_decay=0.05)]
    lr = S.head_lr(0.1, 512, 0.7)
    assert lr == float(np.float32(0.1 * 512 / 256.0 * 0.7))
    one = S.sweep_step(W, b, [mu_w], [mu_b], rm, rv, x, lab, grid, 0.7, cfg)
    want = R.probe_step(W[0], b[0], mu_w, mu_b, rm, rv, x, lab, lr, cfg)
    assert np.array_equal(one["bn"]["y"], want["bn"]["y"]) and np.array_equal(one["bn"]["running_var"], want["bn"]["running_var"])
    h = one["heads"][0]
    for k in ("logits", "dW", "db"):
        assert np.array_equal(h["head"][k], want["head"][k])
    assert h["head"]["loss"] == want["head"]["loss"] and h["head"]["correct"] == want["head"]["correct"]
    for part, ref in (("lars_w", want["lars_w"]), ("lars_b", want["lars_b"])):
        assert np.array_equal(h[part]["p"], ref["p"]) and np.array_equal(h[part]["mu"], ref["mu"]) and h[part]["q"] == ref["q"]


def test_reference_heads_are_independent_and_differ_by_hyper_parameters_only():
    r = np.random.default_rng(5)
    B, D, C, G = 8, 8, 3, 3
    x, lab = R.gen_bn(B, D), r.integers(0, C, B)
    W1, b1 = S.gen_heads(1, C, D)
    W, b = [W1[0]] * G, [b1[0]] * G
    zeros_w, zeros_b = [np.zeros(C * D)] * G, [np.zeros(C)] * G
    cfg = dict(bn_eps=1e-6, bn_momentum=0.1, momentum=0.9, trust_coefficient=0.001, batch_size=256)
    grid = [dict(base_learning_rate=0.1, weight_decay=0.0), dict(base_learning_rate=0.2, weight_decay=0.0), dict(base_learning_rate=0.1, weight_decay=0.1)]
    out = S.sweep_step(W, b, zeros_w, zeros_b, np.zeros(D), np.ones(D), x, lab, grid, 1.0, cfg)
    h = out["heads"]
    assert all(np.array_equal(h[0]["head"]["dW"], h[g]["head"]["dW"]) for g in range(G))    # the same start: the same gradients
    step = lambda g: h[g]["lars_w"]["p"] - W1[0].reshape(-1)
    assert np.allclose(step(1), 2.0 * step(0), rtol=1e-6, atol=0) and not np.allclose(step(2), step(0), rtol=1e-3, atol=0)
    assert np.allclose(h[1]["lars_b"]["p"] - b1[0], 2.0 * (h[0]["lars_b"]["p"] - b1[0]), rtol=1e-6, atol=0)
    assert np.array_equal(h[2]["lars_b"]["p"], h[0]["lars_b"]["p"])                          # the bias takes no weight decay
    # pack / unpack: the stacked layout, padding zero
    flat = S.pack(W, b)
    assert flat.shape == (G, S.head_floats(C, D)) == (G, 28) and np.all(flat[:, C * D + C:] == 0.0)
    Wb, bb = S.unpack(flat, C, D)
    assert all(np.array_equal(Wb[g], W[g]) and np.array_equal(bb[g], b[g]) for g in range(G))
    assert S.head_floats(10, 148) == 1492 and S.head_floats(10, 148) > 10 * 148 + 10          # a shape whose segment has padding


# ---- the sweep's host state -------------------------------------------------------------------------------------------------
def test_sweep_state_on_the_host():
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe, ProbeHead, ProbeSweep
    grid = [dict(base_learning_rate=0.1, weight_decay=0.0), dict(base_learning_rate=0.3, weight_decay=0.0005), dict(base_learning_rate=1.0, weight_decay=0.0)]
    a = ProbeSweep(16, 5, grid, dict(batch_size=512), seed=3)
    proto = ProbeHead(16, 5, 0.01, seed=3)
    assert len(a) == 3 and a.flat.shape == (3, 88) and all(torch.equal(a.flat[g], proto.flat) for g in range(3))   # every head starts as ProbeHead(seed)
    assert np.array_equal(a.head_lrs(0.5), np.array([0.1 * 2 * 0.5, 0.3 * 2 * 0.5, 1.0 * 2 * 0.5]).astype(np.float32))
    a.flat.normal_()
    a.mu.normal_()
    a.bn.running_mean.normal_()
    a.steps, a.epoch = 7, 2
    b = ProbeSweep(16, 5, grid, dict(batch_size=512), seed=4)
    b.load_state_dict(a.state_dict())
    assert torch.equal(a.flat, b.flat) and torch.equal(a.mu, b.mu) and torch.equal(a.bn.running_mean, b.bn.running_mean) and (b.steps, b.epoch) == (7, 2)
    with pytest.raises(ValueError, match="grid"):
        ProbeSweep(16, 5, grid[:2], dict(batch_size=512)).load_state_dict(a.state_dict())
    with pytest.raises(ValueError, match="grid"):
        ProbeSweep(16, 5, grid, dict(batch_size=512)).load_state_dict(LinearProbe(16, 5).state_dict())
    p = a.export(1)
    assert isinstance(p, LinearProbe) and torch.equal(p.head.flat, a.flat[1]) and torch.equal(p.mu, a.mu[1])
    assert torch.equal(p.head.bn.running_mean, a.bn.running_mean) and (p.cfg["base_learning_rate"], p.cfg["weight_decay"]) == (0.3, 0.0005)
    assert (p.steps, p.epoch) == (7, 2) and p.head.flat.data_ptr() != a.flat.data_ptr()
    with pytest.raises(IndexError):
        a.export(3)
    with pytest.raises(ValueError, match="64"):
        ProbeSweep(16, 5, [dict(base_learning_rate=0.01 * (i + 1), weight_decay=0.0) for i in range(65)])
    with pytest.raises(RuntimeError, match="MI355X"):
        a.step(torch.zeros(4, 16), torch.zeros(4, dtype=torch.int64), 1.0)   # no CPU fallback


def test_sweep_scratch_bytes_limits():
    from ssrl_vit_mae_jepa_amd._lib import lib
    assert lib.mae_probe_sweep_scratch_bytes(2000, 384, 10, 8) > 0
    for rows, dim, C, G in ((8, 6, 4, 2), (8, 1028, 4, 2), (8, 16, 1, 2), (8, 16, 129, 2), (8, 16, 4, 0), (8, 16, 4, 65), (0, 16, 4, 2), (2 ** 31 // 8, 16, 4, 2)):
        assert lib.mae_probe_sweep_scratch_bytes(rows, dim, C, G) == -1
