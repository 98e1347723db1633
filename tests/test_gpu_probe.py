"""The linear probe end to end on the MI355X: LinearProbe.step against the fp64 restatement of tests/probe_ref.py over three steps,
evaluate and the folded head, the classifier checkpoint read back through train_mae.build_module, and the CLI in both modes."""
import json
import math

import numpy as np
import pytest
import torch
import yaml

import tests.test_gpu_classifier as TC
from oracle import mae_oracle as O
from tests import probe_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

MICRO = TC.MICRO
CFG = dict(bn_eps=1e-6, bn_momentum=0.1, momentum=0.9, weight_decay=0.0, trust_coefficient=0.001, head_init_std=0.01)
LR = 0.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def np_(t):
    return t.detach().cpu().numpy()


def state_of(probe):
    lin, bn = probe.head.classification.classification, probe.head.bn
    return dict(flat=np_(probe.head.flat).copy(), W=np_(lin.weight).copy(), b=np_(lin.bias).copy(), mu=np_(probe.mu).copy(),
                rm=np_(bn.running_mean).copy(), rv=np_(bn.running_var).copy(), tracked=int(bn.num_batches_tracked))


def within(name, got, want, bound, fails):
    ratio, i = R.worst(got, want, bound)
    print(f"  {name}: worst error / bound {ratio:.3g}")
    if not ratio <= 1.0:
        fails.append(f"{name}: error / bound {ratio:.3g} at flat index {i}")


@pytest.mark.parametrize("B,D,C", [(7, 144, 10), (64, 384, 100)])
def test_three_steps_then_evaluate_and_fold(dev, B, D, C):
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe
    probe = LinearProbe(D, C, CFG, seed=5, device=dev)
    nw, r = C * D, np.random.default_rng([B, D, C])
    fails = []
    for step in range(3):
        x = R.gen_bn(B, D, seed=step)
        labels = r.integers(0, C, B)
        before = state_of(probe)
        loss, correct = probe.step(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev), LR)
        torch.cuda.synchronize()
        after, last, grads = state_of(probe), {k: np_(v) for k, v in probe.last.items()}, np_(probe.grads).copy()
        ref = R.probe_step(before["W"], before["b"], before["mu"][:nw], before["mu"][nw:nw + C], before["rm"], before["rv"], x, labels, LR, CFG)
        print(f"step {step} ({B}, {D}, {C}):")
        # BatchNorm, inside its bounds
        bb = R.bn_train_bounds(ref["bn"], B, D, before["rm"], before["rv"], CFG["bn_eps"], CFG["bn_momentum"])
        for name, got, key in (("y", last["y"], "y"), ("mean", last["mean"], "mean"), ("rstd", last["rstd"], "rstd"),
                               ("running_mean", after["rm"], "running_mean"), ("running_var", after["rv"], "running_var")):
            within(name, got, ref["bn"][key], bb[key], fails)
        assert after["tracked"] == before["tracked"] + 1
        # the head: the figure tests/test_gpu_soft_head.py holds this kernel to in fp32
        h = ref["head"]
        errs = dict(logits=rel_err(torch.from_numpy(last["logits"]), torch.from_numpy(h["logits"])),
                    dW=rel_err(torch.from_numpy(grads[:nw]), torch.from_numpy(h["dW"].reshape(-1))),
                    db=rel_err(torch.from_numpy(grads[nw:nw + C]), torch.from_numpy(h["db"])), loss=abs(float(loss) - h["loss"]) / abs(h["loss"]))
        print("  head rel_err " + " ".join(f"{k} {v:.3e}" for k, v in errs.items()))
        for k, v in errs.items():
            if not v < 1e-5:
                fails.append(f"step {step} {k}: rel_err {v:.3e}")
        assert int(correct) == int((last["logits"].argmax(1) == labels).sum())   # exact on the GPU's own logits
        assert np.all(grads[nw + C:] == 0.0)
        # LARS on the gradients the GPU formed, inside its bounds
        lw = R.lars_step(before["flat"][:nw], grads[:nw], before["mu"][:nw], 1, LR, CFG["momentum"], CFG["weight_decay"], CFG["trust_coefficient"])
        lb = R.lars_step(before["flat"][nw:], grads[nw:], before["mu"][nw:], 0, LR, CFG["momentum"], CFG["weight_decay"], CFG["trust_coefficient"])
        bw, bbias = R.lars_bounds(lw, nw), R.lars_bounds(lb, before["flat"].size - nw)
        within("W'", after["flat"][:nw], lw["p"], bw["p"], fails)
        within("mu_W'", after["mu"][:nw], lw["mu"], bw["mu"], fails)
        within("b'", after["flat"][nw:], lb["p"], bbias["p"], fails)
        within("mu_b'", after["mu"][nw:], lb["mu"], bbias["mu"], fails)
        assert np.all(after["flat"][nw + C:] == 0.0) and np.all(after["mu"][nw + C:] == 0.0)   # the padding stays zero
        assert lw["q"] != 1.0
    assert not fails, "\n".join(fails)

    # evaluate: the running statistics, no state change
    st = state_of(probe)
    x = R.gen_bn(B + 3, D, seed=9)
    labels = r.integers(0, C, B + 3)
    logits, loss, correct = probe.evaluate(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev))
    torch.cuda.synchronize()
    again = state_of(probe)
    assert all(np.array_equal(st[k], again[k]) for k in ("flat", "mu", "rm", "rv")) and again["tracked"] == 3
    ev = R.bn_eval(x, st["rm"], st["rv"], CFG["bn_eps"])
    evb = R.bn_eval_bounds(ev)
    within("evaluate y", np_(probe.last["y"]), ev["y"], evb["y"], fails)
    want = R.head(ev["y"], st["W"], st["b"], labels)
    within("evaluate logits", np_(logits), want["logits"], R.linear_bound(ev["y"], st["W"], st["b"], evb["y"]), fails)
    assert abs(float(loss) - want["loss"]) < 1e-5 * max(1.0, want["loss"]) and int(correct) == int((np_(logits).argmax(1) == labels).sum())
    assert probe.evaluate(torch.from_numpy(x).to(dev))[1] is None

    # the folded head on the raw features: the same logits, inside its own (wider: b' cancels sum W' mean) bound
    wf, bf = probe.folded_head()
    w64, b64 = R.fold(st["W"], st["b"], st["rm"], st["rv"], CFG["bn_eps"])
    assert np.array_equal(np_(wf), w64.astype(np.float32)) and np.array_equal(np_(bf), b64.astype(np.float32))
    flat = torch.zeros((C * D + C + 3) // 4 * 4)
    flat[:nw], flat[nw:nw + C] = wf.reshape(-1), bf
    out = torch.empty(B + 3, C, device=dev)
    need = lib.mae_classifier_head_scratch_bytes(B + 3, C, D)
    scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    from ssrl_vit_mae_jepa_amd._lib import MAE_F32, POOL_CLS, check
    from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream
    xd, fd = torch.from_numpy(x).to(dev), flat.to(dev)
    check(lib.mae_classifier_head(_ptr(xd), MAE_F32, B + 3, 1, D, POOL_CLS, _ptr(fd), C, None, 1.0, _ptr(out), None, None, None, None, _ptr(scratch),
                                  need, _stream(dev)))
    torch.cuda.synchronize()
    fb = R.linear_bound(x, np_(wf), np_(bf)) + R.SECOND * R.U * (np.abs(x.astype(np.float64)) @ np.abs(w64).T + np.abs(b64))
    within("folded logits", np_(out), want["logits"], fb, fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------------
# through the engine
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pool,with_cls", [("cls", True), ("mean", True), ("mean", False)])
def test_checkpoint_reads_back_through_build_module(dev, tmp_path, pool, with_cls):
    from scripts.training.train_mae import build_module
    from ssrl_vit_mae_jepa_amd.classifier import encoder_mae
    from ssrl_vit_mae_jepa_amd.probe import CLASSIFIER_POOL, LinearProbe
    mc = TC.micro_cfg("fp32")
    mae = encoder_mae(mc)
    params = O.init_params(MICRO, 73)
    O.randomize_params(params, seed=5)
    mae.load_state_dict(params)
    mae = mae.to(dev)
    vit = mae.encoder.vit
    vit.with_cls = with_cls
    g = torch.Generator().manual_seed(3)
    images = torch.randint(0, 256, (24, MICRO.in_chans, MICRO.image_size, MICRO.image_size), generator=g, dtype=torch.uint8).to(dev)
    labels = torch.randint(0, 10, (24,), generator=g).to(dev)
    feats = vit.extract_features(images, pool=pool, normalize="none", with_cls=with_cls)
    probe = LinearProbe(MICRO.embed_dim, 10, CFG, seed=5, device=dev)
    for _ in range(2):
        probe.step(feats, labels, LR)
    ck = probe.classifier_checkpoint(vit, mc, pool, epoch=1)
    path = tmp_path / "probe.ckpt"
    torch.save(ck, path)
    model = {k: dict(v) for k, v in mc.items()}
    model["general"].pop("engine_precision")                     # a YAML names the precision under engine:
    cfg = dict(model=model, train={}, engine=dict(precision="fp32"))
    module = build_module(cfg, classifier_ckpt=str(path)).to(dev)
    assert module.model.pool_type == CLASSIFIER_POOL[pool] and module.model.with_cls is with_cls
    logits = module.model.evaluate(images)[0]
    torch.cuda.synchronize()
    wf, bf = probe.folded_head()
    f64 = np_(feats).astype(np.float64)
    want = f64 @ np_(wf).astype(np.float64).T + np_(bf).astype(np.float64)
    bound = 1e-4 * np.abs(f64).max() * np.abs(np_(wf).astype(np.float64)).sum(1).max()
    err = np.abs(np_(logits).astype(np.float64) - want).max()
    print(f"{pool} with_cls {with_cls}: max logit error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    if not with_cls:
        with pytest.raises(ValueError, match="class token"):
            probe.classifier_checkpoint(vit, mc, "cls")


# ------------------------------------------------------------------------------------------------------------------
# the CLI
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", ["none", "crop"])
def test_cli(dev, tmp_path, augment):
    from pathlib import Path
    from scripts.evaluation import evaluate_classifier, linear_probe
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe
    root = Path(__file__).resolve().parents[1]
    cfg = yaml.safe_load((root / "configs" / "vits8_dec192_linprobe.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    argv = ["--config", str(cfg_path), "--checkpoint", "random", "--synthetic_images", "64", "--batch_size", "32", "--output_dir_suffix", "t"]
    res = linear_probe.main(argv + ["--max_epochs", "2"] + (["--augment", "crop"] if augment == "crop" else []))
    out = tmp_path / "outputs" / "probe" / "t"
    for name in ("logs/metrics.jsonl", "checkpoints/best.ckpt", "checkpoints/last.ckpt", "checkpoints/probe_last.pt", "probe.json", "config.yaml"):
        assert (out / name).exists(), name
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2 and [x["epoch"] for x in lines] == [0, 1]
    for x in lines:
        assert set(x) >= {"train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s"}
        assert all(math.isfinite(float(x[k])) for k in ("train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s"))
    assert lines[0]["lr"] == pytest.approx(0.1 * 32 / 256 * 0.1) and res["augment"] == augment   # warm-up epoch 0 of 10
    pj = json.loads((out / "probe.json").read_text())
    assert math.isfinite(pj["test_acc"]) and math.isfinite(pj["test_loss"]) and pj["train_size"] == 50
    ck = torch.load(out / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["with_cls"] is True and ck["hyper_parameters"]["model_cfg"]["head"]["pool"] == "cls"
    # the probe's own state restores bit for bit
    state = torch.load(out / "checkpoints" / "probe_last.pt", map_location="cpu", weights_only=False)
    p = LinearProbe(384, 10, device=dev)
    p.load_state_dict(state)
    assert torch.equal(p.mu.cpu(), state["mu"]) and float(state["mu"].abs().max()) > 0 and (p.steps, p.epoch) == (4, 2)
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        assert torch.equal(getattr(p.head.bn, k).cpu(), state["head.bn." + k])
    assert torch.equal(p.head.classification.classification.weight.cpu(), state["head.classification.classification.weight"])
    if augment == "none":
        linear_probe.main(argv + ["--max_epochs", "1", "--resume", str(out / "checkpoints" / "probe_last.pt")])
        lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
        assert [x["epoch"] for x in lines] == [0, 1, 2]
        kept = json.loads((out / "probe.json").read_text())
        assert kept["best_epoch"] == 0 or lines[2]["val_acc"] > lines[0]["val_acc"]   # a resumed run replaces best.ckpt only by a better epoch
        evaluate_classifier.main(["--config", str(cfg_path), "--checkpoint", str(out / "checkpoints" / "best.ckpt"), "--synthetic_images", "25"])
        ev = json.loads((tmp_path / "outputs" / "test" / "default" / "metrics.json").read_text())
        assert math.isfinite(ev["test_acc"]) and math.isfinite(ev["test_loss"]) and ev["images"] == 25
