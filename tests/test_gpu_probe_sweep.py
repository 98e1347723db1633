"""The linear-probe sweep end to end on the MI355X: ProbeSweep.step against the fp64 restatement (tests/probe_sweep_ref.py) per head over
three steps with the bounds tests/test_gpu_probe.py holds the single probe to, evaluate, export and its classifier checkpoint, the state
round trip bit for bit, and the CLI with a grid."""
import json
import math

import numpy as np
import pytest
import torch
import yaml

import tests.test_gpu_classifier as TC
from oracle import mae_oracle as O
from tests import probe_ref as R
from tests import probe_sweep_ref as S
from tests.util import rel_err

pytestmark = pytest.mark.gpu

MICRO = TC.MICRO
CFG = dict(bn_eps=1e-6, bn_momentum=0.1, momentum=0.9, trust_coefficient=0.001, head_init_std=0.01, batch_size=512)
GRID = [dict(base_learning_rate=lr, weight_decay=wd) for lr in (0.1, 0.3) for wd in (0.0, 0.001)]   # 2 x 2
FACTOR = 0.7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


def state_of(sweep):
    return dict(flat=np_(sweep.flat).copy(), mu=np_(sweep.mu).copy(), rm=np_(sweep.bn.running_mean).copy(), rv=np_(sweep.bn.running_var).copy(),
                tracked=int(sweep.bn.num_batches_tracked))


def within(name, got, want, bound, fails):
    ratio, i = R.worst(got, want, bound)
    print(f"  {name}: worst error / bound {ratio:.3g}")
    if not ratio <= 1.0:
        fails.append(f"{name}: error / bound {ratio:.3g} at flat index {i}")


@pytest.mark.parametrize("B,D,C", [(7, 144, 10), (64, 384, 100)])
def test_three_steps_then_evaluate_and_export(dev, B, D, C):
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe, ProbeHead, ProbeSweep
    sweep = ProbeSweep(D, C, GRID, CFG, seed=5, device=dev)
    G, nw, HF = len(GRID), C * D, S.head_floats(C, D)
    assert all(torch.equal(sweep.flat[g].cpu(), ProbeHead(D, C, 0.01, seed=5).flat) for g in range(G))
    r = np.random.default_rng([B, D, C, 1])
    fails = []
    for step in range(3):
        x = R.gen_bn(B, D, seed=step)
        labels = r.integers(0, C, B)
        before = state_of(sweep)
        loss, correct = sweep.step(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), FACTOR)
        assert loss.shape == (G,) and correct.shape == (G,) and loss.is_cuda and correct.dtype == torch.int32
        torch.cuda.synchronize()
        after, last, grads = state_of(sweep), {k: np_(v) for k, v in sweep.last.items()}, np_(sweep.grads).copy()
        W, b = S.unpack(before["flat"], C, D)
        ref = S.sweep_step(W, b, [before["mu"][g, :nw] for g in range(G)], [before["mu"][g, nw:nw + C] for g in range(G)], before["rm"],
                           before["rv"], x, labels, GRID, FACTOR, CFG)
        print(f"step {step} ({B}, {D}, {C}) x {G} heads:")
        # the shared BatchNorm, inside its bounds
        bb = R.bn_train_bounds(ref["bn"], B, D, before["rm"], before["rv"], CFG["bn_eps"], CFG["bn_momentum"])
        for name, got, key in (("y", last["y"], "y"), ("mean", last["mean"], "mean"), ("rstd", last["rstd"], "rstd"),
                               ("running_mean", after["rm"], "running_mean"), ("running_var", after["rv"], "running_var")):
            within(name, got, ref["bn"][key], bb[key], fails)
        assert after["tracked"] == before["tracked"] + 1
        for g in range(G):
            h, lr, wd = ref["heads"][g]["head"], ref["heads"][g]["lr"], GRID[g]["weight_decay"]
            errs = dict(logits=rel_err(torch.from_numpy(last["logits"][g]), torch.from_numpy(h["logits"])),
                        dW=rel_err(torch.from_numpy(grads[g, :nw]), torch.from_numpy(h["dW"].reshape(-1))),
                        db=rel_err(torch.from_numpy(grads[g, nw:nw + C]), torch.from_numpy(h["db"])),
                        loss=abs(float(loss[g]) - h["loss"]) / abs(h["loss"]))
            print(f"  head {g} rel_err " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
            for k, v in errs.items():
                if not v < 1e-5:
                    fails.append(f"step {step} head {g} {k}: rel_err {v:.3e}")
            assert int(correct[g]) == int((last["logits"][g].argmax(1) == labels).sum())   # exact on the GPU's own logits
            assert np.all(grads[g, nw + C:] == 0.0)
            # LARS on the gradients the GPU formed, with the head's own lr and weight decay, inside its bounds
            lw = R.lars_step(before["flat"][g, :nw], grads[g, :nw], before["mu"][g, :nw], 1, lr, CFG["momentum"], wd, CFG["trust_coefficient"])
            lb = R.lars_step(before["flat"][g, nw:], grads[g, nw:], before["mu"][g, nw:], 0, lr, CFG["momentum"], wd, CFG["trust_coefficient"])
            bw, bbias = R.lars_bounds(lw, nw), R.lars_bounds(lb, HF - nw)
            within(f"head {g} W'", after["flat"][g, :nw], lw["p"], bw["p"], fails)
            within(f"head {g} mu_W'", after["mu"][g, :nw], lw["mu"], bw["mu"], fails)
            within(f"head {g} b'", after["flat"][g, nw:], lb["p"], bbias["p"], fails)
            within(f"head {g} mu_b'", after["mu"][g, nw:], lb["mu"], bbias["mu"], fails)
            assert np.all(after["flat"][g, nw + C:] == 0.0) and np.all(after["mu"][g, nw + C:] == 0.0)   # the padding stays zero
            assert lw["q"] != 1.0
        if step == 0:   # the same start and the same gradients: the heads part by their hyper-parameters alone
            assert np.array_equal(grads[0], grads[1]) and np.array_equal(grads[0], grads[3])
            assert not np.array_equal(after["flat"][0], after["flat"][1]) and not np.array_equal(after["flat"][0], after["flat"][2])
    assert not fails, "\n".join(fails)

    # evaluate: the running statistics, every head, no state change
    st = state_of(sweep)
    x = R.gen_bn(B + 3, D, seed=9)
    labels = r.integers(0, C, B + 3)
    xd, ld = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    logits, loss, correct = sweep.evaluate(xd, ld)
    torch.cuda.synchronize()
    again = state_of(sweep)
    assert all(np.array_equal(st[k], again[k]) for k in ("flat", "mu", "rm", "rv")) and again["tracked"] == 3
    ev = R.bn_eval(x, st["rm"], st["rv"], CFG["bn_eps"])
    evb = R.bn_eval_bounds(ev)
    W, b = S.unpack(st["flat"], C, D)
    assert sweep.evaluate(xd)[1] is None
    for g in range(len(GRID)):
        want = R.head(ev["y"], W[g], b[g], labels)
        bound = R.linear_bound(ev["y"], W[g], b[g], evb["y"])
        within(f"evaluate head {g} logits", np_(logits[g]), want["logits"], bound, fails)
        assert abs(float(loss[g]) - want["loss"]) < 1e-5 * max(1.0, want["loss"]) and int(correct[g]) == int((np_(logits[g]).argmax(1) == labels).sum())
        # export(g): a LinearProbe of its own that gives head g's logits (the same fp64 value, inside the same bound) and carries its state
        probe = sweep.export(g)
        assert isinstance(probe, LinearProbe) and np.array_equal(np_(probe.head.flat), st["flat"][g]) and np.array_equal(np_(probe.mu), st["mu"][g])
        assert np.array_equal(np_(probe.head.bn.running_mean), st["rm"]) and int(probe.head.bn.num_batches_tracked) == 3
        pl, ploss, pcorrect = probe.evaluate(xd, ld)
        torch.cuda.synchronize()
        within(f"export({g}) logits", np_(pl), want["logits"], bound, fails)
        assert np.abs(np_(pl).astype(np.float64) - np_(logits[g])).max() <= 2.0 * bound.max()
        assert abs(float(ploss) - float(loss[g])) < 1e-5 * max(1.0, want["loss"])
    assert all(np.array_equal(st[k], state_of(sweep)[k]) for k in ("flat", "mu", "rm", "rv"))   # export copies
    assert not fails, "\n".join(fails)


def test_state_round_trip_is_bit_exact(dev):
    from ssrl_vit_mae_jepa_amd.probe import ProbeSweep
    B, D, C = 33, 148, 10
    r = np.random.default_rng(8)
    batches = [(torch.from_numpy(R.gen_bn(B, D, seed=s)).to(dev), torch.from_numpy(r.integers(0, C, B)).to(dev)) for s in range(3)]
    a = ProbeSweep(D, C, GRID, CFG, seed=5, device=dev)
    for x, y in batches[:2]:
        a.step(x, y, FACTOR)
    a.epoch = 1
    state = a.state_dict()
    b = ProbeSweep(D, C, GRID, CFG, seed=6, device=dev)
    b.load_state_dict(state)
    la, ca = a.step(*batches[2], 0.9)
    lb, cb = b.step(*batches[2], 0.9)
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(ca, cb) and torch.equal(a.flat, b.flat) and torch.equal(a.mu, b.mu)
    assert torch.equal(a.bn.running_mean, b.bn.running_mean) and torch.equal(a.bn.running_var, b.bn.running_var)
    assert int(b.bn.num_batches_tracked) == 3 and (b.steps, b.epoch) == (3, 1) and float(a.mu.abs().max()) > 0
    with pytest.raises(ValueError, match="grid"):
        ProbeSweep(D, C, GRID[:3], CFG, device=dev).load_state_dict(state)


def test_export_checkpoint_reads_back_through_build_module(dev, tmp_path):
    from scripts.training.train_mae import build_module
    from ssrl_vit_mae_jepa_amd.classifier import encoder_mae
    from ssrl_vit_mae_jepa_amd.probe import ProbeSweep
    mc = TC.micro_cfg("fp32")
    mae = encoder_mae(mc)
    params = O.init_params(MICRO, 73)
    O.randomize_params(params, seed=5)
    mae.load_state_dict(params)
    mae = mae.to(dev)
    vit = mae.encoder.vit
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (24, MICRO.in_chans, MICRO.image_size, MICRO.image_size), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 10, (24,), generator=g).to(dev)
    feats = vit.extract_features(images, pool="cls", normalize="none", with_cls=True)
    sweep = ProbeSweep(MICRO.embed_dim, 10, GRID, CFG, seed=5, device=dev)
    for _ in range(2):
        sweep.step(feats, labels, FACTOR)
    head = 3
    probe = sweep.export(head)
    path = tmp_path / "probe.ckpt"
    torch.save(probe.classifier_checkpoint(vit, mc, "cls", epoch=1), path)
    model = {k: dict(v) for k, v in mc.items()}
    model["general"].pop("engine_precision")
    module = build_module(dict(model=model, train={}, engine=dict(precision="fp32")), classifier_ckpt=str(path)).to(dev)
    logits = module.model.evaluate(images)[0]
    torch.cuda.synchronize()
    wf, bf = probe.folded_head()
    f64 = np_(feats).astype(np.float64)
    want = f64 @ np_(wf).astype(np.float64).T + np_(bf).astype(np.float64)
    bound = 1e-4 * np.abs(f64).max() * np.abs(np_(wf).astype(np.float64)).sum(1).max()   # test_gpu_probe.py's bound for this read-back
    err = np.abs(np_(logits).astype(np.float64) - want).max()
    print(f"export({head}) through build_module: max logit error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    # and they are head 3's logits: the sweep's own evaluation of the same images agrees to the folding's rounding
    own = np_(sweep.evaluate(feats)[0][head]).astype(np.float64)
    assert np.abs(own - want).max() <= bound


# ------------------------------------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", ["none", "crop"])
def test_cli_sweep(dev, tmp_path, augment):
    from pathlib import Path
    from scripts.evaluation import evaluate_classifier, linear_probe
    from ssrl_vit_mae_jepa_amd.probe import ProbeSweep, select
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load((root / "configs" / "vits8_dec192_linprobe.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    argv = ["--config", str(cfg_path), "--checkpoint", "random", "--synthetic_images", "200", "--output_dir_suffix", "s", "--sweep_lr", "0.05,0.1",
            "--sweep_wd", "0,0.001"]
    res = linear_probe.main(argv + ["--max_epochs", "2"] + (["--augment", "crop"] if augment == "crop" else []))
    out = tmp_path / "outputs" / "probe" / "s"
    for name in ("logs/metrics.jsonl", "checkpoints/best.ckpt", "checkpoints/last.ckpt", "checkpoints/probe_last.pt", "probe.json", "sweep.json", "config.yaml"):
        assert (out / name).exists(), name
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert [x["epoch"] for x in lines] == [0, 1]
    for x in lines:   # per-head lists
        for k in ("train_loss", "train_acc", "val_loss", "val_acc", "lr"):
            assert len(x[k]) == 4 and all(math.isfinite(float(v)) for v in x[k]), k
        assert x["leader"] == select(x["val_acc"], x["val_loss"])
    n_train = res["train_size"]
    assert lines[0]["lr"] == [float(np.float32(b * 2000 / 256 * 0.1)) for b in (0.05, 0.05, 0.1, 0.1)]   # warm-up epoch 0 of 10, per head
    sj = json.loads((out / "sweep.json").read_text())
    rows = sj["heads"]
    assert len(rows) == 4 and [(h["base_learning_rate"], h["weight_decay"]) for h in rows] == [(0.05, 0.0), (0.05, 0.001), (0.1, 0.0), (0.1, 0.001)]
    for g, h in enumerate(rows):
        assert h["index"] == g and h["best_epoch"] in (0, 1) and math.isfinite(h["test_acc"]) and math.isfinite(h["test_loss"])
        assert h["best_val_acc"] == max(x["val_acc"][g] for x in lines) == lines[h["best_epoch"]]["val_acc"][g]
        assert h["best_val_loss"] == lines[h["best_epoch"]]["val_loss"][g]
    w = sj["winner"]
    assert w == select([h["best_val_acc"] for h in rows], [h["best_val_loss"] for h in rows])
    pj = json.loads((out / "probe.json").read_text())
    assert pj["sweep_index"] == w == res["sweep_index"] and pj["sweep_heads"] == 4 and pj["augment"] == augment and n_train == pj["train_size"]
    assert (pj["val_acc"], pj["best_epoch"], pj["test_acc"], pj["test_loss"]) == (rows[w]["best_val_acc"], rows[w]["best_epoch"], rows[w]["test_acc"],
                                                                                  rows[w]["test_loss"])
    ck = torch.load(out / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["with_cls"] is True and ck["hyper_parameters"]["model_cfg"]["head"]["pool"] == "cls" and ck["epoch"] == rows[w]["best_epoch"]
    # the whole sweep's state restores; the last checkpoint is the last epoch's leader
    state = torch.load(out / "checkpoints" / "probe_last.pt", map_location="cpu", weights_only=False)
    sweep = ProbeSweep(384, 10, state["grid"], state["cfg"], device=dev)
    sweep.load_state_dict(state)
    assert torch.equal(sweep.flat.cpu(), state["flat"]) and float(state["mu"].abs().max()) > 0 and (sweep.steps, sweep.epoch) == (2, 2)
    last = torch.load(out / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=True)
    wf, bf = sweep.export(lines[1]["leader"]).folded_head()
    assert torch.equal(last["state_dict"]["model.head.classification.weight"], wf) and torch.equal(last["state_dict"]["model.head.classification.bias"], bf)
    if augment == "none":
        # best.ckpt loads in evaluate_classifier's loader; a resume with another grid is refused, with the same grid it continues
        evaluate_classifier.main(["--config", str(cfg_path), "--checkpoint", str(out / "checkpoints" / "best.ckpt"), "--synthetic_images", "25"])
        ev = json.loads((tmp_path / "outputs" / "test" / "default" / "metrics.json").read_text())
        assert math.isfinite(ev["test_acc"]) and math.isfinite(ev["test_loss"]) and ev["images"] == 25
        resume = ["--resume", str(out / "checkpoints" / "probe_last.pt"), "--max_epochs", "1"]
        with pytest.raises(SystemExit) as e:
            linear_probe.main(argv[:-4] + ["--sweep_lr", "0.05,0.2", "--sweep_wd", "0,0.001"] + resume)
        assert "grid" in str(e.value)
        linear_probe.main(argv + resume)
        assert [json.loads(x)["epoch"] for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()] == [0, 1, 2]


def test_cli_refuses_65_heads_before_loading_data(dev, tmp_path, monkeypatch):
    from pathlib import Path
    from scripts.evaluation import linear_probe
    root = Path(__file__).resolve().parents[1]
    monkeypatch.setattr(linear_probe.C, "get_train_batches", lambda *a, **k: (_ for _ in ()).throw(AssertionError("data was loaded")))
    lrs = ",".join(str(0.01 * (i + 1)) for i in range(13))
    with pytest.raises(SystemExit) as e:
        linear_probe.main(["--config", str(root / "configs" / "vits8_dec192_linprobe.yaml"), "--checkpoint", "random", "--synthetic_images", "200",
                           "--sweep_lr", lrs, "--sweep_wd", "0,0.1,0.2,0.3,0.4"])
    assert "65 heads" in str(e.value) and "at most 64" in str(e.value)
