"""Stochastic depth (drop path) through the engine on the MI355X: the scaled classifier step against tests/droppath_ref.py under
autograd, the soft call bit for bit when no table (or an all-ones table) is given, the refusal of a table on the linear probe, the
module's fused step with train.drop_path, and the CLI flag."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import tests.test_gpu_classifier as TC
import tests.test_gpu_patch_classifier as TP
from oracle import mae_oracle as O
from tests import droppath_ref as DR
from tests import mix_ref as R
from tests.util import rel_err, stream

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MICRO = TC.MICRO     # depth 2, D 48, 17 rows per image (16 without the class token)
B = 6
_r = TC._r
K9, K8 = float(torch.tensor(1 / 0.9, dtype=torch.float32)), float(torch.tensor(1 / 0.8, dtype=torch.float32))
# rows: blocks.0 attention, blocks.0 MLP, blocks.1 attention, blocks.1 MLP; columns: images.  Image 0 is dropped in every branch, image 1
# in a single one (blocks.1 MLP); the rest are ones and 1 / (1 - p) values
TABLE = torch.tensor([[0.0, 1.0, 1.0, K9, 1.0, 2.0],
                      [0.0, 1.0, K9, 1.0, 0.0, 1.0],
                      [0.0, 1.0, K8, 0.0, 1.0, K8],
                      [0.0, 0.0, 1.0, K8, K8, 2.0]], dtype=torch.float32)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda", 0)


def soft_batch(step):
    g = torch.Generator().manual_seed(40 + step)
    images = O.synthetic_images(B, MICRO, seed=20 + step)
    ya, yb = torch.randint(0, 10, (B,), generator=g), torch.randint(0, 10, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    return images, ya, yb, lam


def ref_loss_and_grads(p, cfg, images, ya, yb, lam, eps, scale, names, with_cls, pool, bf):
    """tests/test_gpu_soft_classifier.py::ref_soft_loss_and_grads with the encoder of tests/droppath_ref.py."""
    leaves = {k: v.clone().requires_grad_(k in names) for k, v in p.items()}
    op = {("encoder.vit." + k[len("encoder."):]): v.float() for k, v in leaves.items() if k.startswith("encoder.")}
    n, L = images.shape[0], cfg.sequence_length
    if with_cls:
        feats = DR.forward_encoder(op, cfg, images.float(), scale, bf16=bf)
        pooled = feats[:, 0] if pool == "cls" else feats.mean(dim=1) if pool == "mean" else feats[:, 1:].mean(dim=1)
    else:
        pooled = DR.forward_encoder(op, cfg, images.float(), scale, idx_keep=torch.arange(1, L).repeat(n, 1), bf16=bf).mean(dim=1)
    logits = F.linear(_r(pooled, bf), _r(leaves["head.classification.weight"].float(), bf), leaves["head.classification.bias"].float())
    loss = R.soft_loss(logits, ya, yb, lam, eps)
    loss.backward()
    grads = {k: (leaves[k].grad.detach().double() if leaves[k].grad is not None else torch.zeros_like(p[k])) for k in names}
    return loss.detach(), grads


CASES = [(mode, precision, with_cls, pool) for mode in ("last1", "full") for precision in ("fp32", "bf16")
         for with_cls, pool in ((True, "cls"), (True, "mean"), (False, "mean_patches"))]


@pytest.mark.parametrize("mode,precision,with_cls,pool", CASES)
def test_scaled_step_matches_reference(dev, mode, precision, with_cls, pool):
    bf = precision == "bf16"
    mod, params = TP.build_module(dev, precision, mode, with_cls, pool, MICRO)
    names = TC.trainable_names(mod)
    unused = {"encoder.cls_token"} if not with_cls else set()
    p = TC.ref_step_state(mod, params)
    tl, tg = (2e-2, 5e-2) if bf else (1e-4, 2e-4)  # TC.test_two_steps_match_reference
    images, ya, yb, lam = soft_batch(1)
    loss, _correct = mod.loss_and_grads(images.to(dev), ya.to(dev), labels_b=yb.to(dev), lam=lam.to(dev), label_smoothing=0.1, branch_scale=TABLE)
    torch.cuda.synchronize()
    gn = TC.native_grads(mod)
    lref, gref = ref_loss_and_grads(p, MICRO, images, ya, yb, lam, 0.1, TABLE, names, with_cls, pool, bf)
    # the table matters: the all-ones reference's gradients are far outside the tolerance (0.70 to 0.99 here, on the CPU)
    _lones, gones = ref_loss_and_grads(p, MICRO, images, ya, yb, lam, 0.1, torch.ones_like(TABLE), names, with_cls, pool, bf)
    assert rel_err(gones["encoder.blocks.1.mlp.fc2.weight"], gref["encoder.blocks.1.mlp.fc2.weight"]) > 0.3
    errs = {n: rel_err(gn[n], gref[n]) for n in names if n not in unused}
    worst = max(errs, key=errs.get)
    print(f"{mode} {precision} {pool}: loss {abs(float(loss) - float(lref)) / abs(float(lref)):.3e}; worst gradient {worst} {errs[worst]:.3e}")
    assert abs(float(loss) - float(lref)) <= tl * abs(float(lref)), (float(loss), float(lref))
    for n, e in errs.items():
        assert e < tg, (n, e)
    # a table already on the device is the same call
    loss2, _ = mod.loss_and_grads(images.to(dev), ya.to(dev), labels_b=yb.to(dev), lam=lam.to(dev), label_smoothing=0.1, branch_scale=TABLE.to(dev))
    assert torch.equal(loss2, loss)
    with pytest.raises(ValueError):
        mod.loss_and_grads(images.to(dev), ya.to(dev), branch_scale=TABLE[:, :5])


def _raw_call(mod, dev, images, labels, with_cls, pool, train_blocks, train_embed, which, table=None, fill=None):
    """One call of _soft (NULL / NULL / 0) or _sd through the C ABI into fresh outputs -> (rc, [grads, head_g, pos_g, logits, loss, correct])."""
    from ssrl_vit_mae_jepa_amd._lib import lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    clf, m = mod.model, mod.model.mae
    ws = clf.workspace(B)
    head_g, pos_g = mod._grad_buffers()
    m.flat_grads.zero_(); head_g.fill_(7.0); pos_g.fill_(7.0)
    loss, correct = torch.full((1,), -3.0, device=dev), torch.full((1,), -3, dtype=torch.int32, device=dev)
    logits = torch.full((B, 10), -3.0, device=dev)
    head = (m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B)
    mid = (int(with_cls), TP.POOL[pool], 10, train_blocks, train_embed, 1.0, _ptr(ws), ws.numel(), _ptr(m.flat_grads), _ptr(head_g), _ptr(pos_g),
           _ptr(logits), _ptr(loss), _ptr(correct))
    if which == "soft":
        rc = lib.mae_engine_classifier_loss_and_grads_soft(*head, *mid, None, None, 0.0, stream(dev))
    else:
        rc = lib.mae_engine_classifier_loss_and_grads_sd(*head, *mid, None, None, 0.0, _ptr(table), stream(dev))
    torch.cuda.synchronize()
    return rc, [t.clone() for t in (m.flat_grads, head_g, pos_g, logits, loss, correct)]


@pytest.mark.parametrize("with_cls,pool", [(True, "cls"), (True, "mean"), (False, "mean_patches")])
def test_no_table_and_all_ones_equal_the_soft_call_in_every_bit(dev, with_cls, pool):
    from ssrl_vit_mae_jepa_amd._lib import check
    mod, _ = TP.build_module(dev, "bf16", "full", with_cls, pool, MICRO)
    images = O.synthetic_images(B, MICRO, seed=8).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    ones = torch.ones(2 * MICRO.depth, B, device=dev)
    outs = []
    for which, table in (("soft", None), ("sd", None), ("sd", ones)):
        rc, out = _raw_call(mod, dev, images, labels, with_cls, pool, 2, 1, which, table)
        check(rc)
        outs.append(out)
    for other in outs[1:]:
        for a, b in zip(outs[0], other):
            assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # and a table with a zero in it is another result
    rc, out = _raw_call(mod, dev, images, labels, with_cls, pool, 2, 1, "sd", TABLE.to(dev))
    check(rc)
    assert not torch.equal(out[0], outs[0][0]) and not torch.equal(out[4], outs[0][4])


def test_table_on_the_linear_probe_is_refused_before_any_launch(dev):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    mod, _ = TP.build_module(dev, "bf16", "frozen", True, "cls", MICRO)
    images = O.synthetic_images(B, MICRO, seed=8).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    rc, out = _raw_call(mod, dev, images, labels, True, "cls", -1, 0, "sd", torch.ones(2 * MICRO.depth, B, device=dev))
    check(0)
    assert rc != 0 and b"branch_scale" in lib.mae_last_error()
    grads, head_g, pos_g, logits, loss, correct = out
    assert float(grads.abs().max()) == 0.0 and (head_g == 7.0).all() and (pos_g == 7.0).all()
    assert (logits == -3.0).all() and float(loss) == -3.0 and int(correct) == -3
    rc, out = _raw_call(mod, dev, images, labels, True, "cls", -1, 0, "sd", None)   # without a table the probe runs as before
    check(rc)
    assert math.isfinite(float(out[4]))
    with pytest.raises(ValueError):                                                     # the module says the same
        mod.loss_and_grads(images, labels, branch_scale=torch.ones(2 * MICRO.depth, B))


def _fused_run(dev, rate, steps=3, epochs=2):
    g = torch.Generator().manual_seed(2)
    images = (torch.rand(24, 3, MICRO.image_size, MICRO.image_size, generator=g) * 255).to(torch.uint8)
    labels = torch.arange(24) % 10
    mod, _ = TP.build_module(dev, "bf16", "full", True, "mean_patches", MICRO)
    mod.drop_path = rate
    with torch.no_grad():
        val0 = mod.validation_step((images.to(dev), labels.to(dev)), 0).clone()
    losses = []
    for epoch in range(epochs):
        mod.current_epoch = epoch
        for _ in range(steps):
            loss, _c = mod.fused_training_step(images.to(dev), labels.to(dev), lr=2e-3)
            losses.append(loss.clone())
    torch.cuda.synchronize()
    return mod, val0.cpu(), torch.cat(losses).cpu(), mod.model.mae.flat_params.clone()


def test_fused_steps_with_drop_path_are_deterministic(dev):
    """train.drop_path = 0.5 through fused_training_step: equal (seed, epoch, step) give equal bits, the rate changes the run, and
    validation does not see the rate (evaluation never drops)."""
    a = _fused_run(dev, 0.5)
    b = _fused_run(dev, 0.5)
    off = _fused_run(dev, 0.0)
    assert a[0]._drop_step == 6 and off[0]._drop_step == 0
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert torch.isfinite(a[2]).all() and torch.isfinite(a[3]).all()
    assert not torch.equal(a[2], off[2]) and not torch.equal(a[3], off[3])
    assert torch.equal(a[1], off[1])                  # the same weights validate to the same loss whatever the rate
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path
    t = draw_drop_path(MICRO.depth, 24, 0.5, (73, 0, 0))
    assert (t[:2] == 1).all() and (t[2:] == 0).any() and (t[2:] == 2).any()   # the first step's draw drops and keeps
    # training_step (loss and gradients only) draws the same way
    mod, _ = TP.build_module(dev, "bf16", "full", True, "mean_patches", MICRO)
    mod.drop_path = 0.5
    imgs, labels = O.synthetic_images(B, MICRO, seed=3).to(dev), torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    l1 = mod.training_step((imgs, labels), 0).clone()
    want, _ = mod.loss_and_grads(imgs, labels, branch_scale=draw_drop_path(MICRO.depth, B, 0.5, (73, 0, 0)))
    assert mod._drop_step == 1 and torch.equal(l1, want[0])
    # the linear probe ignores the rate: the same bits as rate 0
    probe, _ = TP.build_module(dev, "bf16", "frozen", True, "cls", MICRO)
    base = probe.training_step((imgs, labels), 0).clone()
    probe.drop_path = 0.5
    assert torch.equal(probe.training_step((imgs, labels), 0), base) and probe._drop_step == 0


def test_cli_finetune_with_drop_path(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg["train"].update(batch_size=128, learning_rate=1e-3, warmup_epochs=1, freeze_encoder=False)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, "-m", "scripts.training.train_mae", "--config", str(cfg_path), "--synthetic_images", "300", "--max_epochs", "1",
                        "--drop_path", "0.2"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "outputs" / "train" / "mae_finetune"
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 1
    assert all(math.isfinite(lines[0][k]) for k in ("train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s")), lines[0]
    assert yaml.safe_load((out / "config.yaml").read_text())["train"]["drop_path"] == 0.2
    ck = torch.load(out / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["training_cfg"]["drop_path"] == 0.2
