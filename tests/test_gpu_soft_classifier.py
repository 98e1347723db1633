"""The fine-tuning recipe through the engine on the MI355X: the soft-target step against the oracle's autograd in every
trainable mode, the hard call bit for bit when nothing soft is asked for, layer-wise learning-rate decay against per-group
AdamW, the tensors that must keep their bits, the mixed fused step and the CLI."""
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
from tests import mix_ref as R
from tests.util import rel_err, stream

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MICRO = TC.MICRO
B = 6
_r = TC._r


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
    lam[0], lam[1], yb[2] = 0.0, 1.0, ya[2]
    return images, ya, yb, lam


def ref_soft_loss_and_grads(p, cfg, images, ya, yb, lam, eps, names, with_cls, pool, bf):
    """TC.ref_loss_and_grads / TP.ref_loss_and_grads (the oracle's encoder under autograd) with the loss replaced by the
    soft-target loss.  A tensor that takes no part in the forward comes back with a zero gradient."""
    leaves = {k: v.clone().requires_grad_(k in names) for k, v in p.items()}
    op = {("encoder.vit." + k[len("encoder."):]): v.float() for k, v in leaves.items() if k.startswith("encoder.")}
    n, L = images.shape[0], cfg.sequence_length
    if with_cls:
        feats = O.forward_encoder(op, cfg, images.float(), bf16=bf)
        pooled = feats[:, 0] if pool == "cls" else feats.mean(dim=1) if pool == "mean" else feats[:, 1:].mean(dim=1)
    else:
        pooled = O.forward_encoder(op, cfg, images.float(), idx_keep=torch.arange(1, L).repeat(n, 1), bf16=bf).mean(dim=1)
    logits = F.linear(_r(pooled, bf), _r(leaves["head.classification.weight"].float(), bf), leaves["head.classification.bias"].float())
    loss = R.soft_loss(logits, ya, yb, lam, eps)
    loss.backward()
    grads = {k: (leaves[k].grad.detach().double() if leaves[k].grad is not None else torch.zeros_like(p[k])) for k in names}
    return loss.detach(), grads


SOFT_CASES = [(mode, precision, True, "cls") for mode in ("frozen", "last1", "full") for precision in ("fp32", "bf16")] + \
             [("full", "fp32", True, "mean"), ("full", "bf16", False, "mean_patches")]


@pytest.mark.parametrize("mode,precision,with_cls,pool", SOFT_CASES)
def test_soft_step_matches_reference(dev, mode, precision, with_cls, pool):
    bf = precision == "bf16"
    mod, params = TP.build_module(dev, precision, mode, with_cls, pool, MICRO)
    names = TC.trainable_names(mod)
    unused = {"encoder.cls_token"} if not with_cls else set()
    p = TC.ref_step_state(mod, params)
    tl, tg = (2e-2, 5e-2) if bf else (1e-4, 2e-4)  # TC.test_two_steps_match_reference
    for step, eps in ((1, 0.1), (2, 0.0)):
        images, ya, yb, lam = soft_batch(step)
        loss, correct = mod.loss_and_grads(images.to(dev), ya.to(dev), labels_b=yb.to(dev), lam=lam.to(dev), label_smoothing=eps)
        torch.cuda.synchronize()
        gn = TC.native_grads(mod)
        lref, gref = ref_soft_loss_and_grads(p, MICRO, images, ya, yb, lam, eps, names, with_cls, pool, bf)
        errs = {n: rel_err(gn[n], gref[n]) for n in names if n not in unused}
        worst = max(errs, key=errs.get)
        print(f"eps {eps}: loss {abs(float(loss) - float(lref)) / abs(float(lref)):.3e}; worst gradient {worst} {errs[worst]:.3e}")
        assert abs(float(loss) - float(lref)) <= tl * abs(float(lref)), (float(loss), float(lref))
        for n, e in errs.items():
            assert e < tg, (eps, n, e)
        # smoothing alone through the module's configured value is the same call
        if step == 1:
            mod.label_smoothing = eps
            loss2, _ = mod.loss_and_grads(images.to(dev), ya.to(dev), labels_b=yb.to(dev), lam=lam.to(dev))
            mod.label_smoothing = 0.0
            assert torch.equal(loss2, loss)


@pytest.mark.parametrize("with_cls,pool", [(True, "cls"), (True, "mean"), (True, "mean_patches"), (False, "mean_patches")])
def test_nothing_soft_equals_ex_in_every_bit(dev, with_cls, pool):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    mod, _ = TP.build_module(dev, "bf16", "full", with_cls, pool, MICRO)
    clf, m = mod.model, mod.model.mae
    images = O.synthetic_images(B, MICRO, seed=8).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    outs = []
    for soft in (False, True):
        ws = clf.workspace(B)
        head_g, pos_g = mod._grad_buffers()
        m.flat_grads.zero_(); head_g.fill_(7.0); pos_g.fill_(7.0)
        loss, correct = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        logits = torch.empty(B, 10, device=dev)
        head = (m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B)
        mid = (int(with_cls), TP.POOL[pool], 10, 2, 1, 1.0, _ptr(ws), ws.numel(), _ptr(m.flat_grads), _ptr(head_g), _ptr(pos_g), _ptr(logits),
               _ptr(loss), _ptr(correct))
        if soft:
            check(lib.mae_engine_classifier_loss_and_grads_soft(*head, *mid, None, None, 0.0, stream(dev)))
        else:
            check(lib.mae_engine_classifier_loss_and_grads_ex(*head, *mid, stream(dev)))
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (m.flat_grads, head_g, pos_g, logits, loss, correct)])
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # the module takes the hard route when nothing is active, the soft one otherwise: same loss to rounding at lam = 1, eps = 0
    hard, _ = mod.loss_and_grads(images, labels)
    assert torch.equal(hard, outs[0][4])
    one, _ = mod.loss_and_grads(images, labels, lam=torch.ones(B, device=dev))
    assert abs(float(one) - float(hard)) <= 1e-6 * abs(float(hard))
    ws = clf.workspace(B)
    rc = lib.mae_engine_classifier_loss_and_grads_soft(*head, *mid[:6], _ptr(ws), ws.numel(), *mid[8:], None, None, 1.0, stream(dev))
    check(0)
    assert rc != 0 and b"label_smoothing" in lib.mae_last_error()


def layer_groups(mod, names):
    """name -> lr scale: embeddings 0, blocks.i -> i + 1, norm and the head depth + 1."""
    out = {}
    for n in names:
        layer = mod.layer_of("head") if n.startswith("head.") else mod.layer_of(n[len("encoder."):])
        out[n] = mod.layer_scale(layer)
    return out


@pytest.mark.parametrize("mode,precision,with_cls,pool", [("full", "fp32", True, "cls"), ("full", "bf16", True, "cls"), ("last1", "fp32", True, "cls"),
                                                          ("full", "fp32", False, "mean_patches")])
def test_layer_decay_two_steps_match_per_group_adamw(dev, mode, precision, with_cls, pool):
    bf, lr, decay = precision == "bf16", 1e-3, 0.5
    mod, params = TP.build_module(dev, precision, mode, with_cls, pool, MICRO)
    mod.layer_decay = decay
    m = mod.model.mae
    names = TC.trainable_names(mod)
    unused = {"encoder.cls_token"} if not with_cls else set()
    scales = layer_groups(mod, names)
    assert scales["head.classification.weight"] == 1.0 and scales["encoder.norm.weight"] == 1.0
    if mode == "full":
        assert scales["encoder.pos_embed"] == decay ** 3 and scales["encoder.blocks.0.attn.qkv.weight"] == decay ** 2
    p = TC.ref_step_state(mod, params)
    p0 = {k: v.clone() for k, v in p.items()}
    arena0 = m.flat_params.clone()
    state = {}
    for step in (1, 2):
        images, ya, yb, lam = soft_batch(step)
        mod.loss_and_grads(images.to(dev), ya.to(dev), labels_b=yb.to(dev), lam=lam.to(dev), label_smoothing=0.1)
        mod.optimizer_step(lr)
        _lref, gref = ref_soft_loss_and_grads(p, MICRO, images, ya, yb, lam, 0.1, names, with_cls, pool, bf)
        gref = {k: v.clone() for k, v in gref.items() if k not in unused}
        O.clip_grad_norm(gref, 1.0)  # one norm over the whole trainable set, as before
        for scale in sorted(set(scales.values())):  # one AdamW group per layer, its own learning rate
            group = [k for k in gref if scales[k] == scale]
            pp = {k: p[k] for k in group}
            O.adamw_step(pp, {k: gref[k] for k in group}, state, lr * scale, step, weight_decay=0.05)
            p.update(pp)
        if not with_cls and "encoder.pos_embed" in names:
            p["encoder.pos_embed"][:, 0] = p0["encoder.pos_embed"][:, 0]
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in mod.model.state_dict().items()}
    tp = 2e-2 if bf else 2e-5  # the existing two-step parameter tolerance
    D = MICRO.embed_dim
    for n in names:
        if n in unused:
            continue
        a, b = sd[n], p[n]
        if n.endswith("attn.qkv.bias"):  # the key part's exact gradient is zero (tests/test_gpu_classifier.py)
            a, b = torch.cat([a[:D], a[2 * D:]]), torch.cat([b[:D], b[2 * D:]])
        assert rel_err(a, b) < tp, (n, rel_err(a, b))
        assert not torch.equal(sd[n], p0[n]), n
        # the size of the update is the group's: with one learning rate for all, a layer-0 update would be 8x too large (error 7).
        # fp32, matrices and pos_embed only (where a gradient is rounding noise AdamW takes lr-sized steps of either sign)
        if not bf and (n.endswith("weight") and sd[n].dim() >= 2 or n == "encoder.pos_embed"):
            assert rel_err(sd[n] - p0[n], p[n] - p0[n]) < 0.5, (n, rel_err(sd[n] - p0[n], p[n] - p0[n]))
    if mode == "full" and not with_cls:  # never read, never decayed: the same bits
        assert torch.equal(mod.model.encoder.cls_token.detach().cpu(), params["encoder.vit.cls_token"])
        assert torch.equal(mod.model.encoder.pos_embed.detach().cpu()[:, 0], params["encoder.vit.pos_embed"][:, 0])
    if mode != "full":  # frozen tensors keep their bits
        for name, off, numel, _s, _f in m.engine.table:
            if name.startswith("encoder.vit.") and "encoder." + name[len("encoder.vit."):] not in names:
                assert torch.equal(m.flat_params[off:off + numel], arena0[off:off + numel]), name


@pytest.mark.parametrize("mode,with_cls,pool", [("full", True, "cls"), ("last1", True, "cls"), ("frozen", True, "cls"), ("full", False, "mean_patches")])
def test_layer_decay_one_is_the_plain_step_bit_for_bit(dev, mode, with_cls, pool):
    """optimizer_step at layer_decay = 1 against the step as it was before layer decay existed, issued here call by call
    (``plain_optimizer_step``): the same arena, bf16 operand copies, head, pos_embed and optimizer state after two steps."""
    images, ya, _yb, _lam = soft_batch(1)
    lr = 1e-3
    results = []
    for plain in (True, False):
        mod, _ = TP.build_module(dev, "bf16", mode, with_cls, pool, MICRO)
        assert mod.layer_decay == 1.0
        for _ in range(2):
            mod.loss_and_grads(images.to(dev), ya.to(dev))
            if plain:
                plain_optimizer_step(mod, lr, dev)
            else:
                mod.optimizer_step(lr)
        torch.cuda.synchronize()
        m = mod.model.mae
        results.append([m.flat_params.clone(), m._weights().clone(), mod.model.head.flat.clone()] + [mod._opt[k].clone() for k in sorted(mod._opt)])
        assert {"head_m", "head_v", "stats"} <= set(mod._opt) and ("arena_m" in mod._opt) == (mode != "frozen")
    assert len(results[0]) == len(results[1])
    for a, b in zip(*results):
        assert torch.equal(a, b)


def plain_optimizer_step(mod, lr, dev):
    """The optimizer step with one learning rate, as a sequence of C calls: sum of squares and clip, one mae_engine_adamw_range
    per piece of _update_ranges at lr, the head and pos_embed buffers at lr, then the transposed-copy refresh."""
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    tb, te = mod.train_mode()
    clf, m = mod.model, mod.model.mae
    h, s = m.engine.handle, stream(dev)
    head_g, pos_g = mod._grad_buffers()
    lo, hi = mod._arena_range(tb, te)
    n_arena = m.engine.trainable_elems
    stats, sums, scratch = mod._state("stats", 8, dev), mod._state("sumsq", 4, dev), m._scratch_f32()
    mod._opt_steps += 1
    step = mod._opt_steps
    hyper = (float(lr), 0.9, 0.999, 1e-8, float(mod.weight_decay))
    if hi > lo:
        check(lib.mae_engine_grad_sumsq_range(h, _ptr(m.flat_grads), lo, hi - lo, _ptr(sums), _ptr(scratch), s))
    check(lib.mae_engine_grad_sumsq_buffer(h, _ptr(head_g), head_g.numel(), int(hi > lo), _ptr(sums), _ptr(scratch), s))
    if te:
        check(lib.mae_engine_grad_sumsq_buffer(h, _ptr(pos_g), pos_g.numel(), 1, _ptr(sums), _ptr(scratch), s))
    check(lib.mae_engine_clip_from_sumsq(h, _ptr(sums), 1.0, _ptr(stats), s))
    pieces, pos_row0 = mod._update_ranges(tb, te)
    for p_lo, p_n in pieces:
        ea, eq = mod._state("arena_m", n_arena, dev), mod._state("arena_v", n_arena, dev)
        check(lib.mae_engine_adamw_range(h, _ptr(m.flat_params), _ptr(m.flat_grads), _ptr(ea), _ptr(eq), _ptr(m._weights()), *hyper, step,
                                         _ptr(stats), p_lo, p_n, s))
    check(lib.mae_engine_adamw_buffer(h, _ptr(clf.head.flat), _ptr(head_g), _ptr(mod._state("head_m", head_g.numel(), dev)),
                                      _ptr(mod._state("head_v", head_g.numel(), dev)), head_g.numel(), *hyper, step, _ptr(stats), s))
    if te:
        _n, pos_off, pos_n, _s, _f = m._offsets["encoder.vit.pos_embed"]
        skip = pos_row0 * m._dims["embed_dim"]
        check(lib.mae_engine_adamw_buffer(h, _ptr(m.flat_params[pos_off + skip:pos_off + pos_n]), _ptr(pos_g[skip:]),
                                          _ptr(mod._state("pos_m", pos_n, dev)[skip:]), _ptr(mod._state("pos_v", pos_n, dev)[skip:]),
                                          pos_n - skip, *hyper, step, _ptr(stats), s))
    if hi > lo:
        check(lib.mae_engine_refresh_transposed_range(h, _ptr(m.flat_params), _ptr(m._weights()), lo, hi - lo, s))
    m.mark_weights_fresh()


def test_mixed_fused_steps_are_deterministic_and_train(dev):
    """mixup + CutMix + smoothing + layer decay through fused_training_step on uint8 images: the same (seed, epoch, step) gives
    the same bits, both kinds of batch occur and every loss is finite; evaluation stays hard-label."""
    cfg = MICRO
    g = torch.Generator().manual_seed(2)
    images = (torch.rand(24, 3, cfg.image_size, cfg.image_size, generator=g) * 255).to(torch.uint8)
    labels = torch.arange(24) % 10
    for c in range(10):
        images[labels == c, c % 3, (c * 3):(c * 3 + 3)] = 255
    runs = []
    for _ in range(2):
        mod, _ = TP.build_module(dev, "bf16", "full", True, "mean_patches", cfg)
        mod.label_smoothing, mod.mixup_alpha, mod.cutmix_alpha, mod.layer_decay = 0.1, 0.8, 1.0, 0.75
        losses = []
        for epoch in range(2):
            mod.current_epoch = epoch
            for _step in range(8):
                loss, correct = mod.fused_training_step(images.to(dev), labels.to(dev), lr=2e-3)
                losses.append(loss.clone())
                assert 0 <= int(correct) <= 24
        torch.cuda.synchronize()
        runs.append((torch.cat(losses).cpu(), mod.model.mae.flat_params.clone()))
        assert mod._mix_step == 16
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.isfinite(runs[0][0]).all()
    from ssrl_vit_mae_jepa_amd.data import draw_mix_params
    kinds = {draw_mix_params(24, cfg.image_size, (73, s // 8, s), 0.8, 1.0, 1.0, 0.5).cutmix for s in range(16)}  # the draws of the run
    assert kinds == {True, False}
    # evaluation stays hard-label: it equals F.cross_entropy of its own logits
    with torch.no_grad():
        logits, loss, correct = mod.model.evaluate(images.to(dev), labels.to(dev))
    assert abs(float(loss) - float(F.cross_entropy(logits.cpu().double(), labels))) <= 1e-5 * float(loss)


def test_cli_finetune_with_the_recipe(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg["train"].update(batch_size=128, learning_rate=1e-3, warmup_epochs=1, freeze_encoder=False)
    cfg["test"]["batch_size"] = 256
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True, timeout=600)  # noqa: E731
    r = run("scripts.training.train_mae", "--config", str(cfg_path), "--synthetic_images", "600", "--max_epochs", "2",
            "--label_smoothing", "0.1", "--mixup", "0.8", "--cutmix", "1.0", "--layer_decay", "0.75")
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "outputs" / "train" / "mae_finetune"
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    for rec in lines:
        assert all(math.isfinite(rec[k]) for k in ("train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s")), rec
        assert 0.0 <= rec["train_acc"] <= 1.0 and rec["train_loss"] > 0
    saved = yaml.safe_load((out / "config.yaml").read_text())["train"]
    assert (saved["label_smoothing"], saved["mixup_alpha"], saved["cutmix_alpha"], saved["layer_decay"]) == (0.1, 0.8, 1.0, 0.75)
    best = out / "checkpoints" / "best.ckpt"
    assert best.exists()
    ck = torch.load(best, map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["training_cfg"]["layer_decay"] == 0.75
    r = run("scripts.evaluation.evaluate_classifier", "--config", str(cfg_path), "--checkpoint", str(best), "--synthetic_images", "500")
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads((tmp_path / "outputs" / "test" / "default" / "metrics.json").read_text())
    assert math.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
