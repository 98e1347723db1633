"""The classifier on patch-only sequences (I-JEPA encoders) and the patch-row mean on the MI355X: the row-range head kernel
vs fp64, the native step against the CPU reference in every trainable mode, the tensors a patch-only encoder never reads,
the old entry points bit for bit, the ViT-S/8 geometry and the CLIs."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import tests.test_gpu_classifier as TC
from oracle import mae_oracle as O
from tests.util import BF16, F32, TDT, rel_err, stream

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MICRO = TC.MICRO                                    # 32 px, patch 8: N = 16 patch rows
ODD = O.MAEConfig(image_size=24, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                  decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)  # N = 9: not a multiple of the four row-loading waves
POOL = {"cls": 0, "mean": 1, "mean_patches": 2}
_r = TC._r


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------------------------
# head kernel through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def run_head_ex(dev, feats, dt, with_cls, pool, head, C, labels, grad_scale=1.0, check_rc=True):
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    B, rows, D = feats.shape
    f = feats.to(dev, TDT[dt]).contiguous()
    h = head.to(dev).contiguous()
    lab = labels.to(dev).contiguous()
    logits = torch.empty(B, C, device=dev)
    loss = torch.empty(1, device=dev)
    correct = torch.empty(1, dtype=torch.int32, device=dev)
    hg = torch.full((C * D + C,), float("nan"), device=dev)
    dfeat = torch.full((B, rows, D), float("nan"), dtype=TDT[dt], device=dev)
    n = lib.mae_classifier_head_scratch_bytes(B, C, D)
    scratch = torch.empty(n, dtype=torch.uint8, device=dev)
    rc = lib.mae_classifier_head_ex(_ptr(f), dt, B, rows, D, with_cls, pool, _ptr(h), C, _ptr(lab), float(grad_scale), _ptr(logits), _ptr(loss),
                                    _ptr(correct), _ptr(hg), _ptr(dfeat), _ptr(scratch), n, stream(dev))
    if not check_rc:
        return rc
    check(rc)
    torch.cuda.synchronize()
    return logits.cpu(), loss.cpu()[0], int(correct.cpu()[0]), hg.cpu(), dfeat.float().cpu()


def head_reference(feats, lo, head, C, labels, bf, grad_scale=1.0):
    """tests/test_gpu_classifier.py::head_reference with the pooled rows [lo, rows): fp64 with the engine's bf16 rounding
    points (feats as stored, pooled, W, d_logits); the rows below lo get a zero gradient."""
    B, rows, D = feats.shape
    x = _r(feats.float(), bf).double()
    pooled = _r(x[:, lo:].mean(dim=1).float(), bf).double()
    W = _r(head[:C * D].view(C, D), bf).double()
    b = head[C * D:C * D + C].double()
    logits = pooled @ W.T + b
    loss = F.cross_entropy(logits, labels)
    dl = (torch.softmax(logits, dim=1) - F.one_hot(labels, C).double()) * grad_scale / B
    dl = _r(dl.float(), bf).double()
    dW, db = dl.T @ pooled, dl.sum(0)
    dfeat = torch.zeros(B, rows, D, dtype=torch.float64)
    dfeat[:, lo:] = ((dl @ W) / (rows - lo))[:, None, :]
    return logits, loss, torch.cat([dW.reshape(-1), db]), dfeat


HEAD_SHAPES = [(1, 1, 2, 4), (1, 2, 2, 4), (7, 17, 10, 384), (7, 9, 128, 1024), (65, 5, 10, 144), (3, 144, 10, 384)]
# every shape with each (with_cls, pool); one row is one patch, so (1, 1, 2, 4) exists without a class token only
HEAD_CASES = [(*shape, with_cls, pool) for shape in HEAD_SHAPES for with_cls, pool in ((0, 1), (0, 2), (1, 2)) if shape[1] > with_cls]
_head_inputs = {}


def head_inputs(B, rows, C, D):
    """One set of inputs (and its two fp64 references per precision) per shape, shared by every combination."""
    key = (B, rows, C, D)
    if key not in _head_inputs:
        g = torch.Generator().manual_seed(B * 131 + rows * 17 + C * 7 + D)
        feats = torch.randn(B, rows, D, generator=g)
        head = torch.cat([torch.randn(C * D, generator=g) * D ** -0.5, torch.randn(C, generator=g) * 0.1])
        labels = torch.randint(0, C, (B,), generator=g)
        _head_inputs[key] = (feats, head, labels, {})
    return _head_inputs[key]


@pytest.mark.parametrize("B,rows,C,D,with_cls,pool", HEAD_CASES)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_head_range_kernel_matches_fp64(dev, B, rows, C, D, with_cls, pool, dt):
    feats, head, labels, refs = head_inputs(B, rows, C, D)
    bf, lo = dt == BF16, 1 if with_cls else 0
    if (lo, bf) not in refs:
        refs[(lo, bf)] = head_reference(feats, lo, head, C, labels, bf, grad_scale=0.5)
    lr, lossr, hgr, dfr = refs[(lo, bf)]
    logits, loss, correct, hg, dfeat = run_head_ex(dev, feats, dt, with_cls, pool, head, C, labels, grad_scale=0.5)
    tol = 2e-3 if bf else 1e-5
    print(f"logits {rel_err(logits, lr):.3e} loss {abs(float(loss) - float(lossr)):.3e} head_grads {rel_err(hg, hgr):.3e} d_feats {rel_err(dfeat, dfr):.3e}")
    assert rel_err(logits, lr) < tol
    assert abs(float(loss) - float(lossr)) <= tol * max(1.0, abs(float(lossr)))
    assert correct == int((logits.argmax(1) == labels).sum())  # exact on the engine's own logits
    assert rel_err(hg, hgr) < (2e-2 if bf else 1e-4)
    assert rel_err(dfeat, dfr) < (2e-2 if bf else 1e-4)
    assert torch.isfinite(dfeat).all()  # every row of d_feats is written
    if with_cls:
        assert torch.equal(dfeat[:, 0], torch.zeros(B, D))  # the class row: exact zeros
    # bit-identical from run to run
    again = run_head_ex(dev, feats, dt, with_cls, pool, head, C, labels, grad_scale=0.5)
    for x, y in zip((logits, loss, correct, hg, dfeat), again):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


@pytest.mark.parametrize("B,rows,C,D", HEAD_SHAPES)
@pytest.mark.parametrize("dt", [F32, BF16])
def test_patch_only_mean_and_mean_patches_are_the_same_bits(dev, B, rows, C, D, dt):
    feats, head, labels, _ = head_inputs(B, rows, C, D)
    a = run_head_ex(dev, feats, dt, 0, POOL["mean"], head, C, labels)
    b = run_head_ex(dev, feats, dt, 0, POOL["mean_patches"], head, C, labels)
    for x, y in zip(a, b):
        assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


def test_head_ex_old_combinations_and_rejections(dev):
    from ssrl_vit_mae_jepa_amd._lib import lib
    feats, head, labels, _ = head_inputs(7, 17, 10, 384)
    # with_cls = 1 and cls / mean: the old kernel, bit for bit (d_feats of cls is (B, D): compare through the old runner's shapes)
    for pool in (0, 1):
        old = TC.run_head(dev, feats, BF16, pool, head, 10, labels)
        new = run_head_ex(dev, feats, BF16, 1, pool, head, 10, labels)
        for i, (x, y) in enumerate(zip(old, new)):
            x, y = torch.as_tensor(x), torch.as_tensor(y)
            if i == 4 and pool == 0:
                y = y.reshape(-1)[:x.numel()].view_as(x)  # the compact (B, D) gradient sits at the front of the buffer
            assert torch.equal(x, y), (pool, i)
    # no class token to pool: refused before any launch
    assert run_head_ex(dev, feats, BF16, 0, POOL["cls"], head, 10, labels, check_rc=False) != 0
    assert b"class token" in lib.mae_last_error()
    one = feats[:, :1].contiguous()
    assert run_head_ex(dev, one, BF16, 1, POOL["mean_patches"], head, 10, labels, check_rc=False) != 0  # seq_len >= 2
    assert run_head_ex(dev, feats, BF16, 2, POOL["mean"], head, 10, labels, check_rc=False) != 0
    assert run_head_ex(dev, feats, BF16, 0, 3, head, 10, labels, check_rc=False) != 0


# ------------------------------------------------------------------------------------------------------------------
# the native step
# ------------------------------------------------------------------------------------------------------------------
def build_module(dev, precision, mode, with_cls, pool, cfg=MICRO, C=10, seed=5):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    mc = TC.micro_cfg(precision, pool, cfg)
    mae = encoder_mae(mc)
    params = O.init_params(cfg, 73)
    O.randomize_params(params, seed=seed)
    mae.load_state_dict(params)
    mae.encoder.vit.with_cls = with_cls
    torch.manual_seed(seed)
    mod = ViTClassifierTrainModule(pretrained_encoder=mae.encoder.vit, model_cfg=mc,
                                   training_cfg=dict(learning_rate=1e-3, weight_decay=0.05, freeze_encoder=True), num_classes=C)
    TC.set_mode(mod, mode)
    return mod.to(dev), params


def ref_loss_and_grads(p, cfg, images, labels, names, with_cls, bf):
    """The oracle's encoder over the patch tokens alone (with_cls False) or over [cls | patches] with the patch-row mean.
    A tensor that takes no part in the forward (cls_token of a patch-only encoder) comes back with a zero gradient."""
    leaves = {k: v.clone().requires_grad_(k in names) for k, v in p.items()}
    op = {("encoder.vit." + k[len("encoder."):]): v.float() for k, v in leaves.items() if k.startswith("encoder.")}
    B, L = images.shape[0], cfg.sequence_length
    if with_cls:
        pooled = O.forward_encoder(op, cfg, images.float(), bf16=bf)[:, 1:].mean(dim=1)
    else:
        pooled = O.forward_encoder(op, cfg, images.float(), idx_keep=torch.arange(1, L).repeat(B, 1), bf16=bf).mean(dim=1)
    logits = F.linear(_r(pooled, bf), _r(leaves["head.classification.weight"].float(), bf), leaves["head.classification.bias"].float())
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    grads = {k: (leaves[k].grad.detach().double() if leaves[k].grad is not None else torch.zeros_like(p[k])) for k in names}
    return loss.detach(), grads, logits.detach()


def two_steps(dev, precision, mode, with_cls, pool, cfg):
    B, lr = 6, 1e-3
    bf = precision == "bf16"
    D = cfg.embed_dim
    mod, params = build_module(dev, precision, mode, with_cls, pool, cfg)
    m = mod.model.mae
    names = TC.trainable_names(mod)
    assert ("encoder.pos_embed" in names) == (mode == "full")
    unused = {"encoder.cls_token"} if not with_cls else set()  # what a patch-only forward never reads (and pos_embed[:, 0])
    p = TC.ref_step_state(mod, params)
    p0 = {k: v.clone() for k, v in p.items()}
    arena0 = m.flat_params.clone()
    state = {}
    g = torch.Generator().manual_seed(11)
    for step in (1, 2):
        images = O.synthetic_images(B, cfg, seed=20 + step)
        labels = torch.randint(0, 10, (B,), generator=g)
        # sentinels where exact zeros are expected (the arena's padding is never written, so it is not filled: it reaches the norm)
        m.named_flat_views(m.flat_grads)["encoder.vit.cls_token"].fill_(float("nan"))
        mod.pos_grads.fill_(float("nan"))
        loss, correct = mod.loss_and_grads(images.to(dev), labels.to(dev))
        torch.cuda.synchronize()
        gn = TC.native_grads(mod)
        lref, gref, _ = ref_loss_and_grads(p, cfg, images, labels, names, with_cls, bf)
        tl, tg = (2e-2, 5e-2) if bf else (1e-4, 2e-4)
        errs = {n: rel_err(gn[n], gref[n]) for n in names if n not in unused}
        worst = max(errs, key=errs.get)
        print(f"step {step}: loss {abs(float(loss) - float(lref)) / abs(float(lref)):.3e}; worst gradient {worst} {errs[worst]:.3e}")
        assert abs(float(loss) - float(lref)) <= tl * abs(float(lref)), (step, float(loss), float(lref))
        for n in names:
            if n in unused:
                continue
            assert rel_err(gn[n], gref[n]) < tg, (step, n, rel_err(gn[n], gref[n]))
        if mode == "full" and not with_cls:  # exact zeros where no token carries a gradient
            assert torch.equal(mod.pos_grads[:D], torch.zeros(D, device=dev))
            assert torch.equal(gn["encoder.cls_token"], torch.zeros(1, 1, D, dtype=torch.float64))
            assert torch.isfinite(mod.pos_grads).all()
        mod.optimizer_step(lr)
        gref = {k: v.clone() for k, v in gref.items()}
        O.clip_grad_norm(gref, 1.0)
        pp = {k: p[k] for k in names if k not in unused}
        O.adamw_step(pp, {k: gref[k] for k in pp}, state, lr, step, weight_decay=0.05)
        p.update(pp)
        if not with_cls and "encoder.pos_embed" in names:
            p["encoder.pos_embed"][:, 0] = p0["encoder.pos_embed"][:, 0]  # the optimizer leaves the unused row alone
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in mod.model.state_dict().items()}
    tp = 2e-2 if bf else 2e-5
    for n in names:
        if n in unused:
            continue
        a, b = sd[n], p[n]
        if n.endswith("attn.qkv.bias"):  # the key part's exact gradient is zero (tests/test_gpu_classifier.py): query / value parts only
            a, b = torch.cat([a[:D], a[2 * D:]]), torch.cat([b[:D], b[2 * D:]])
        assert rel_err(a, b) < tp, (n, rel_err(a, b))
        assert not torch.equal(sd[n], p0[n]), n  # every trainable tensor moved
    if mode == "full":
        pe0 = params["encoder.vit.pos_embed"].double()
        assert float((sd["encoder.pos_embed"] - pe0).abs().max()) > 1e-4
        assert rel_err(sd["encoder.pos_embed"] - pe0, p["encoder.pos_embed"] - pe0) < (1.5e-1 if bf else 1e-3)
        if not with_cls:  # bit-identical after two steps: neither a gradient nor weight decay reached them
            assert torch.equal(mod.model.encoder.cls_token.detach().cpu(), params["encoder.vit.cls_token"])
            assert torch.equal(mod.model.encoder.pos_embed.detach().cpu()[:, 0], params["encoder.vit.pos_embed"][:, 0])
        else:
            assert not torch.equal(mod.model.encoder.cls_token.detach().cpu(), params["encoder.vit.cls_token"])  # here cls_token trains
    else:  # frozen tensors: the same bits as before
        for name, off, numel, _s, _f in m.engine.table:
            if name.startswith("encoder.vit.") and "encoder." + name[len("encoder.vit."):] not in names:
                assert torch.equal(m.flat_params[off:off + numel], arena0[off:off + numel]), name


@pytest.mark.parametrize("mode", TC.MODES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_patch_only_two_steps_match_reference(dev, precision, mode):
    two_steps(dev, precision, mode, False, "mean_patches", MICRO)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_patch_only_two_steps_odd_row_count(dev, precision):
    two_steps(dev, precision, "full", False, "mean", ODD)


@pytest.mark.parametrize("mode", ["frozen", "full"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mean_patches_with_cls_two_steps_match_reference(dev, precision, mode):
    two_steps(dev, precision, mode, True, "mean_patches", MICRO)


def test_patch_only_logits_match_feature_extraction(dev):
    """An independent route to the same logits: the features kernel's patch mean, then the head in fp64."""
    mod, _ = build_module(dev, "fp32", "frozen", False, "mean")
    imgs = O.synthetic_images(5, MICRO, seed=31).to(dev)
    with torch.no_grad():
        logits = mod.model(imgs).double().cpu()
        feats = mod.model.mae.extract_features(imgs, pool="mean", with_cls=False).double().cpu()
    ref = F.linear(feats, mod.model.head.classification.weight.detach().double().cpu(), mod.model.head.classification.bias.detach().double().cpu())
    err = float((logits - ref).abs().max())
    print(f"max |logits - ref| {err:.3e} of {float(ref.abs().max()):.3e}")
    assert err <= 1e-4 * float(ref.abs().max())


@pytest.mark.parametrize("pool", ["cls", "mean"])
def test_ex_with_cls_equals_old_entry_point(dev, pool):
    """with_cls = 1 and cls / mean through the _ex call: the old call's launches, so every output has the same bits."""
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    mod, _ = TC.build_module(dev, "bf16", "full", pool)
    clf, m = mod.model, mod.model.mae
    B = 6
    images = O.synthetic_images(B, MICRO, seed=8).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    assert lib.mae_engine_classifier_workspace_bytes_ex(m.engine.handle, B, 10, 1) == lib.mae_engine_classifier_workspace_bytes(m.engine.handle, B, 10)
    outs = []
    for ex in (False, True):
        ws = clf.workspace(B)
        head_g, pos_g = mod._grad_buffers()
        m.flat_grads.zero_(); head_g.fill_(7.0); pos_g.fill_(7.0)
        loss, correct = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
        logits = torch.empty(B, 10, device=dev)
        head = (m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B)
        tail = (10, 2, 1, 1.0, _ptr(ws), ws.numel(), _ptr(m.flat_grads), _ptr(head_g), _ptr(pos_g), _ptr(logits), _ptr(loss), _ptr(correct), stream(dev))
        if ex:
            check(lib.mae_engine_classifier_loss_and_grads_ex(*head, 1, POOL[pool], *tail))
        else:
            check(lib.mae_engine_classifier_loss_and_grads(*head, POOL[pool], *tail))
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (m.flat_grads, head_g, pos_g, logits, loss, correct)])
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    # and the _ex forward refuses the class pool on a patch-only sequence before any launch
    ws = clf.workspace(B)
    rc = lib.mae_engine_classifier_forward_ex(m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images),
                                              m._img_dt(images), None, B, 0, POOL["cls"], 10, _ptr(ws), ws.numel(), _ptr(outs[0][3]), None, None,
                                              stream(dev))
    assert rc != 0 and b"class token" in lib.mae_last_error()


@pytest.mark.parametrize("pool", ["cls", "mean"])
def test_module_calls_equal_first_entry_points(dev, pool):
    """The Python module always takes the widest entries (loss_and_grads -> _sd, evaluate -> forward_ex).  With nothing extended
    asked for they issue the launches of the first entry points: every output has the bits of the direct narrow C call."""
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    mod, _ = TC.build_module(dev, "bf16", "full", pool)
    clf, m = mod.model, mod.model.mae
    assert not clf.extended and mod.label_smoothing == 0.0
    B = 6
    images = O.synthetic_images(B, MICRO, seed=8).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2, 5], device=dev)
    head_g, pos_g = mod._grad_buffers()
    common = (m.engine.handle, _ptr(m.flat_params), _ptr(m._weights()), _ptr(clf.head.flat), _ptr(images), m._img_dt(images), _ptr(labels), B,
              POOL[pool], 10)
    outs = []
    for through_module in (False, True):
        m.flat_grads.zero_(); head_g.fill_(7.0); pos_g.fill_(7.0)
        logits = torch.empty(B, 10, device=dev)
        if through_module:
            loss, correct = mod.loss_and_grads(images, labels, logits_out=logits)
        else:
            ws = clf.workspace(B)
            loss, correct = torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
            check(lib.mae_engine_classifier_loss_and_grads(*common, 2, 1, 1.0, _ptr(ws), ws.numel(), _ptr(m.flat_grads), _ptr(head_g), _ptr(pos_g),
                                                           _ptr(logits), _ptr(loss), _ptr(correct), stream(dev)))
        torch.cuda.synchronize()
        outs.append([t.clone() for t in (m.flat_grads, head_g, pos_g, logits, loss, correct)])
    for a, b in zip(*outs):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)
    assert float(outs[0][0].abs().max()) > 0 and not torch.equal(outs[0][1], torch.full_like(head_g, 7.0))  # the gradients were written
    # evaluation: ViTClassifier.evaluate against mae_engine_classifier_forward
    ws = clf.workspace(B)
    logits, loss, correct = torch.empty(B, 10, device=dev), torch.empty(1, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.mae_engine_classifier_forward(*common, _ptr(ws), ws.numel(), _ptr(logits), _ptr(loss), _ptr(correct), stream(dev)))
    torch.cuda.synchronize()
    with torch.no_grad():
        got = clf.evaluate(images, labels)
    torch.cuda.synchronize()
    for a, b in zip((logits, loss, correct), got):
        assert torch.isfinite(a.float()).all() and torch.equal(a, b)


def test_vits8_geometry_patch_only_full_mode(dev):
    """96 px, patch 8: 144 rows, depth 12, bf16 -- the MFMA attention and the NT / wgrad ring kernels at T = 144."""
    cfg = O.VIT_S8_YAMLDEC
    B = 3
    mod, params = build_module(dev, "bf16", "full", False, "mean_patches", cfg=cfg, seed=1)
    names = TC.trainable_names(mod)
    images = O.synthetic_images(B, cfg, seed=4)
    labels = torch.tensor([1, 7, 4])
    loss, _c = mod.loss_and_grads(images.to(dev), labels.to(dev))
    torch.cuda.synchronize()
    gn = TC.native_grads(mod)
    lref, gref, _ = ref_loss_and_grads(TC.ref_step_state(mod, params), cfg, images, labels, names, False, True)  # one CPU autograd pass
    errs = {n: rel_err(gn[n], gref[n]) for n in names if n != "encoder.cls_token"}
    worst = max(errs, key=errs.get)
    print(f"loss {abs(float(loss) - float(lref)) / abs(float(lref)):.3e}; worst gradient {worst} {errs[worst]:.3e}")
    assert abs(float(loss) - float(lref)) <= 2e-2 * abs(float(lref))
    for n, e in errs.items():
        assert e < 5e-2, (n, e)
    D = cfg.embed_dim
    assert torch.equal(mod.pos_grads[:D], torch.zeros(D, device=dev))
    assert torch.equal(gn["encoder.cls_token"], torch.zeros(1, 1, D, dtype=torch.float64))


def test_cli_pretrain_ijepa_probe_evaluate(dev, tmp_path):
    import yaml
    from ssrl_vit_mae_jepa_amd.representation import load_eval_encoder
    cfg = yaml.safe_load((ROOT / "configs" / "ijepa_vits8.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg["model"]["encoder"] = dict(embed_dim=144, depth=2, num_heads=6)
    cfg["model"]["predictor"] = dict(pred_embed_dim=96, pred_depth=1, pred_num_heads=6)
    del cfg["model"]["head"]  # an I-JEPA config without model.head: the pool defaults to mean_patches
    cfg["pretrain"].update(batch_size=128, total_epochs=1)
    cfg["train"].update(batch_size=256, learning_rate=1e-3, warmup_epochs=1)
    cfg["test"]["batch_size"] = 256
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True, timeout=900)  # noqa: E731
    r = run("scripts.training.pretrain_ijepa", "--config", str(cfg_path), "--synthetic_images", "256", "--max_epochs", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    enc = tmp_path / "outputs" / "pretrain" / "ijepa_pretrain" / "checkpoints" / "last.ckpt"
    r = run("scripts.training.train_mae", "--config", str(cfg_path), "--encoder_ckpt", str(enc), "--encoder", "target", "--pool", "cls",
            "--synthetic_images", "2000", "--max_epochs", "2")
    assert r.returncode != 0 and "I-JEPA encoders see no class token" in r.stderr
    r = run("scripts.training.train_mae", "--config", str(cfg_path), "--encoder_ckpt", str(enc), "--encoder", "target",
            "--synthetic_images", "2000", "--max_epochs", "2")
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "outputs" / "train" / "mae_finetune"
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 2
    for rec in lines:
        assert all(math.isfinite(rec[k]) for k in ("train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s")), rec
    best = out / "checkpoints" / "best.ckpt"
    ck = torch.load(best, map_location="cpu", weights_only=True)
    assert ck["hyper_parameters"]["with_cls"] is False
    assert ck["hyper_parameters"]["model_cfg"]["head"]["pool"] == "mean_patches"
    r = run("scripts.evaluation.evaluate_classifier", "--config", str(cfg_path), "--checkpoint", str(best), "--synthetic_images", "1000")
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads((tmp_path / "outputs" / "test" / "default" / "metrics.json").read_text())
    assert math.isfinite(res["test_loss"]) and 0.0 <= res["test_acc"] <= 1.0
    # the evaluation tools see a patch-only encoder in the fine-tuned checkpoint
    ev = load_eval_encoder(best, cfg["model"], precision="bf16", device=dev)
    assert (ev.kind, ev.with_cls) == ("classifier", False)
    f = ev.features((torch.rand(4, 3, 96, 96, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev), pool="mean")
    assert f.shape == (4, 144) and torch.isfinite(f).all()
