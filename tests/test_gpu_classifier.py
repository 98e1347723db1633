"""The downstream classifier on the MI355X: head kernel vs fp64, determinism, the native step against the CPU reference
in every trainable mode, frozen tensors untouched, agreement with the autograd hand-off, a full-size run and the CLIs."""
import json
import math
import subprocess
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O
from tests.util import BF16, F32, TDT, rel_err, stream

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda", 0)


def _r(x, bf):
    return x.to(torch.bfloat16).to(torch.float32) if bf else x


# ------------------------------------------------------------------------------------------------------------------
# head kernel through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def run_head(dev, feats, dt, pool, head, C, labels, grad_scale=1.0, grads=True):
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    from ssrl_vit_mae_jepa_amd.mae import _ptr
    B, L, D = feats.shape
    f = feats.to(dev, TDT[dt]).contiguous()
    h = head.to(dev).contiguous()
    lab = labels.to(dev).contiguous()
    logits = torch.empty(B, C, device=dev)
    loss = torch.empty(1, device=dev)
    correct = torch.empty(1, dtype=torch.int32, device=dev)
    hg = torch.full((C * D + C,), float("nan"), device=dev) if grads else None
    dfeat = (torch.empty(B, D, dtype=TDT[dt], device=dev) if pool == _lib.POOL_CLS else torch.empty(B, L, D, dtype=TDT[dt], device=dev)) if grads else None
    n = lib.mae_classifier_head_scratch_bytes(B, C, D)
    scratch = torch.empty(n, dtype=torch.uint8, device=dev)
    check(lib.mae_classifier_head(_ptr(f), dt, B, L, D, pool, _ptr(h), C, _ptr(lab), float(grad_scale), _ptr(logits), _ptr(loss),
                                  _ptr(correct), _ptr(hg), _ptr(dfeat), _ptr(scratch), n, stream(dev)))
    torch.cuda.synchronize()
    return logits.cpu(), loss.cpu()[0], int(correct.cpu()[0]), (hg.cpu() if grads else None), (dfeat.float().cpu() if grads else None)


def head_reference(feats, pool, head, C, labels, bf, grad_scale=1.0):
    """fp64 reference with the engine's bf16 rounding points (feats as stored, pooled, W, d_logits)."""
    B, L, D = feats.shape
    x = _r(feats.float(), bf).double()
    pooled = x[:, 0] if pool == 0 else x.mean(dim=1)
    pooled = _r(pooled.float(), bf).double()
    W = _r(head[:C * D].view(C, D), bf).double()
    b = head[C * D:C * D + C].double()
    logits = pooled @ W.T + b
    loss = F.cross_entropy(logits, labels)
    p = torch.softmax(logits, dim=1)
    dl = (p - F.one_hot(labels, C).double()) * grad_scale / B
    dl = _r(dl.float(), bf).double()
    dW, db = dl.T @ pooled, dl.sum(0)
    dpool = dl @ W
    dfeat = dpool if pool == 0 else (dpool / L)[:, None, :].expand(B, L, D)
    correct = int((logits.argmax(1) == labels).sum())
    return logits, loss, correct, torch.cat([dW.reshape(-1), db]), dfeat


@pytest.mark.parametrize("B,C,D", [(1, 2, 144), (7, 10, 384), (2000, 10, 384), (7, 100, 1024), (2000, 100, 144)])
@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("dt", [F32, BF16])
def test_head_kernel_matches_fp64(dev, B, C, D, pool, dt):
    L = 5 if B == 2000 else 17
    g = torch.Generator().manual_seed(B * 131 + C * 7 + D + pool)
    feats = torch.randn(B, L, D, generator=g)
    head = torch.cat([torch.randn(C * D, generator=g) * D ** -0.5, torch.randn(C, generator=g) * 0.1])
    labels = torch.randint(0, C, (B,), generator=g)
    bf = dt == BF16
    logits, loss, correct, hg, dfeat = run_head(dev, feats, dt, pool, head, C, labels, grad_scale=0.5)
    lr, lossr, correctr, hgr, dfr = head_reference(feats, pool, head, C, labels, bf, grad_scale=0.5)
    tol = 2e-3 if bf else 1e-5
    assert rel_err(logits, lr) < tol
    assert abs(float(loss) - float(lossr)) <= tol * max(1.0, abs(float(lossr)))
    # argmax is exact on the engine's own logits (ties among near-equal float logits may flip only through rounding)
    assert correct == int((logits.argmax(1) == labels).sum())
    if not bf:
        assert correct == correctr
    assert rel_err(hg, hgr) < (2e-2 if bf else 1e-4)
    assert rel_err(dfeat, dfr) < (2e-2 if bf else 1e-4)


def test_head_argmax_tie_and_bad_label(dev):
    B, L, D, C = 4, 3, 8, 5
    feats = torch.zeros(B, L, D)
    head = torch.zeros(C * D + C)
    head[C * D:] = torch.tensor([0.0, 2.0, 2.0, 1.0, 2.0])  # equal maxima at 1, 2, 4: torch picks 1
    labels = torch.tensor([1, 2, 4, 1])
    logits, loss, correct, _hg, _df = run_head(dev, feats, F32, 0, head, C, labels)
    assert int(logits.argmax(1)[0]) == 1 and correct == 2
    assert abs(float(loss) - float(F.cross_entropy(logits, labels))) < 1e-6
    bad = torch.tensor([1, 7, -1, 0])
    _l, loss, correct, hg, _df = run_head(dev, feats, F32, 0, head, C, bad)
    assert math.isnan(float(loss))
    assert correct == 1


def test_head_kernel_is_deterministic(dev):
    g = torch.Generator().manual_seed(3)
    B, L, D, C = 2000, 5, 384, 10
    feats, head = torch.randn(B, L, D, generator=g), torch.randn(C * D + C, generator=g) * 0.05
    labels = torch.randint(0, C, (B,), generator=g)
    for pool in (0, 1):
        a, b = run_head(dev, feats, BF16, pool, head, C, labels), run_head(dev, feats, BF16, pool, head, C, labels)
        for x, y in zip(a, b):
            assert torch.equal(torch.as_tensor(x), torch.as_tensor(y))


# ------------------------------------------------------------------------------------------------------------------
# the native step
# ------------------------------------------------------------------------------------------------------------------
def micro_cfg(precision, pool="cls", cfg=MICRO):
    return dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
                encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                decoder=dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads),
                head=dict(embed_dim=cfg.embed_dim, pool=pool))


def build_module(dev, precision, mode, pool="cls", cfg=MICRO, C=10, seed=5):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    mc = micro_cfg(precision, pool, cfg)
    mae = encoder_mae(mc)
    params = O.init_params(cfg, 73)
    O.randomize_params(params, seed=seed)
    mae.load_state_dict(params)
    torch.manual_seed(seed)
    mod = ViTClassifierTrainModule(pretrained_encoder=mae.encoder.vit, model_cfg=mc,
                                   training_cfg=dict(learning_rate=1e-3, weight_decay=0.05, freeze_encoder=True), num_classes=C)
    set_mode(mod, mode)
    return mod.to(dev), params


def set_mode(mod, mode):
    if mode == "frozen":
        mod.freeze_encoder()
    elif mode == "full":
        mod.unfreeze_encoder()
    else:
        mod.unfreeze_last_layers(int(mode[len("last"):]))


def trainable_names(mod):
    return [n for n, p in mod.model.named_parameters() if p.requires_grad]


def ref_step_state(mod, params):
    """oracle parameters in ViTClassifier naming (encoder.<timm>, head.classification.*)."""
    p = {("encoder." + k[len("encoder.vit."):]): v.clone().double() for k, v in params.items() if k.startswith("encoder.vit.")}
    p["head.classification.weight"] = mod.model.head.classification.weight.detach().cpu().double().clone()
    p["head.classification.bias"] = mod.model.head.classification.bias.detach().cpu().double().clone()
    return p


def ref_loss_and_grads(p, cfg, images, labels, names, pool, bf):
    leaves = {k: v.clone().requires_grad_(k in names) for k, v in p.items()}
    op = {("encoder.vit." + k[len("encoder."):]): v for k, v in leaves.items() if k.startswith("encoder.")}
    feats = O.forward_encoder({k: v.float() for k, v in op.items()}, cfg, images.float(), bf16=bf)
    pooled = feats[:, 0] if pool == "cls" else feats.mean(dim=1)
    logits = F.linear(_r(pooled, bf), _r(leaves["head.classification.weight"].float(), bf), leaves["head.classification.bias"].float())
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return loss.detach(), {k: leaves[k].grad.detach().double() for k in names}, logits.detach()


def native_grads(mod):
    """name -> gradient the native step produced (ViTClassifier naming)."""
    m = mod.model.mae
    out = {}
    views = m.named_flat_views(m.flat_grads)
    for n in trainable_names(mod):
        if n.startswith("head."):
            C, D = mod.model.num_classes, mod.model.head.input_dim
            hg = mod.head_grads.cpu()
            out[n] = hg[:C * D].view(C, D) if n.endswith("weight") else hg[C * D:C * D + C]
        elif n == "encoder.pos_embed":
            out[n] = mod.pos_grads.cpu().view(1, m.sequence_length, -1)
        else:
            out[n] = views["encoder.vit." + n[len("encoder."):]].cpu()
    return {k: v.double() for k, v in out.items()}


MODES = ["frozen", "last0", "last1", "full"]


@pytest.mark.parametrize("pool", ["cls", "mean"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_two_steps_match_reference(dev, precision, mode, pool):
    cfg, B, lr = MICRO, 6, 1e-3
    bf = precision == "bf16"
    mod, params = build_module(dev, precision, mode, pool)
    names = trainable_names(mod)
    assert ("encoder.pos_embed" in names) == (mode == "full")
    p = ref_step_state(mod, params)
    p0 = {k: v.clone() for k, v in p.items()}
    state = {}
    g = torch.Generator().manual_seed(11)
    for step in (1, 2):
        images = O.synthetic_images(B, cfg, seed=20 + step)
        labels = torch.randint(0, 10, (B,), generator=g)
        loss, correct = mod.loss_and_grads(images.to(dev), labels.to(dev))
        torch.cuda.synchronize()
        gn = native_grads(mod)
        lref, gref, _ = ref_loss_and_grads(p, cfg, images, labels, names, pool, bf)
        tl, tg = (2e-2, 5e-2) if bf else (1e-4, 2e-4)
        assert abs(float(loss) - float(lref)) <= tl * abs(float(lref)), (step, float(loss), float(lref))
        for n in names:
            assert rel_err(gn[n], gref[n]) < tg, (step, n, rel_err(gn[n], gref[n]))
        mod.optimizer_step(lr)
        gref = {k: v.clone() for k, v in gref.items()}
        O.clip_grad_norm(gref, 1.0)
        pp = {k: p[k] for k in names}
        O.adamw_step(pp, gref, state, lr, step, weight_decay=0.05)
        p.update(pp)
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu().double() for k, v in mod.model.state_dict().items()}
    tp = 2e-2 if bf else 2e-5  # the existing two-step parity tolerances (tests/test_gpu_engine.py)
    D = cfg.embed_dim
    for n in names:
        a, b = sd[n], p[n]
        if n.endswith("attn.qkv.bias"):
            # the key bias shifts every score of a query row by the same amount: its exact gradient is zero, and AdamW turns
            # the rounding noise of both sides into lr-sized steps of either sign -- compare the query / value parts only
            a, b = torch.cat([a[:D], a[2 * D:]]), torch.cat([b[:D], b[2 * D:]])
        assert rel_err(a, b) < tp, (n, rel_err(a, b))
        assert not torch.equal(sd[n], p0[n]), n  # every trainable tensor moved
    if mode == "full":  # pos_embed trains, and by the reference's amount
        p0 = params["encoder.vit.pos_embed"].double()
        assert float((sd["encoder.pos_embed"] - p0).abs().max()) > 1e-4
        assert rel_err(sd["encoder.pos_embed"] - p0, p["encoder.pos_embed"] - p0) < (1.5e-1 if bf else 1e-3)  # bf16: AdamW magnifies rounding of small gradients


@pytest.mark.parametrize("mode", MODES)
def test_frozen_tensors_untouched_and_bits_repeat(dev, mode):
    mod, _ = build_module(dev, "bf16", mode, "cls")
    m = mod.model.mae
    images = O.synthetic_images(5, MICRO, seed=3).to(dev)
    labels = torch.tensor([0, 3, 9, 2, 2], device=dev)
    # NaN sentinel in every gradient row: the rows of frozen tensors must keep it
    m.flat_grads.fill_(float("nan"))
    mod.loss_and_grads(images, labels)
    torch.cuda.synchronize()
    names = set(trainable_names(mod))
    views = m.named_flat_views(m.flat_grads)
    for k, v in views.items():
        if not k.startswith("encoder.vit."):
            continue
        tn = "encoder." + k[len("encoder.vit."):]
        if tn in names:
            assert torch.isfinite(v).all(), k
        else:
            assert torch.isnan(v).all(), k
    # determinism: a second identical call gives the same bits
    m.flat_grads.zero_()  # (padding between tensors is never written: the sentinel must not reach the norm)
    mod.loss_and_grads(images, labels)
    first = (m.flat_grads.clone(), mod.head_grads.clone(), mod.pos_grads.clone())
    loss_a, _ = mod.loss_and_grads(images, labels)
    la = loss_a.clone()
    loss_b, _ = mod.loss_and_grads(images, labels)
    for a, b in zip(first, (m.flat_grads, mod.head_grads, mod.pos_grads)):
        assert torch.equal(torch.nan_to_num(a, 7.0), torch.nan_to_num(b, 7.0))
    assert torch.equal(la, loss_b)
    # the step changes nothing frozen: arena rows of frozen tensors (and in frozen mode the whole arena + the bf16 copies)
    arena0, wc0 = m.flat_params.clone(), m._weights().clone()
    mod.optimizer_step(1e-3)
    torch.cuda.synchronize()
    for name, off, numel, _s, _f in m.engine.table:
        if not name.startswith("encoder.vit."):
            continue
        tn = "encoder." + name[len("encoder.vit."):]
        same = torch.equal(m.flat_params[off:off + numel], arena0[off:off + numel])
        assert same == (tn not in names), name
    if mode == "frozen":
        assert torch.equal(m.flat_params, arena0) and torch.equal(m._wcache, wc0)


def test_last1_matches_autograd_handoff(dev):
    """unfreeze_last_layers(1), fp32: the fused step's gradients equal those of the existing hand-off (forward_features
    autograd node + torch head + F.cross_entropy) with the same head weights."""
    mod, _ = build_module(dev, "fp32", "last1", "cls")
    m = mod.model.mae
    images = O.synthetic_images(4, MICRO, seed=9).to(dev)
    labels = torch.tensor([1, 0, 7, 7], device=dev)
    loss, _ = mod.loss_and_grads(images, labels)
    torch.cuda.synchronize()
    gn = native_grads(mod)
    for p in mod.model.parameters():
        p.grad = None
    feats = mod.model.encoder.forward_features(images)
    logits = F.linear(feats[:, 0], mod.model.head.classification.weight, mod.model.head.classification.bias)
    lt = F.cross_entropy(logits, labels)
    lt.backward()
    assert abs(lt.item() - float(loss)) <= 1e-5 * abs(lt.item())
    for n, p in mod.model.named_parameters():
        if p.requires_grad:
            assert rel_err(gn[n], p.grad) < 1e-4, n


def test_handoff_refuses_after_classifier_call(dev):
    mod, _ = build_module(dev, "fp32", "last1", "cls")
    images = O.synthetic_images(3, MICRO, seed=2).to(dev)
    feats = mod.model.encoder.forward_features(images)
    mod.loss_and_grads(images, torch.tensor([1, 2, 3], device=dev))
    with pytest.raises(RuntimeError):
        feats.sum().backward()
    with pytest.raises(RuntimeError):
        mod.model(images)  # parameters require grad: an inference call refuses to run under grad
    with torch.no_grad():
        assert mod.model(images).shape == (3, 10)


def test_vits8_full_mode_b2000(dev):
    cfg = O.VIT_S8_YAMLDEC
    mod, params = build_module(dev, "bf16", "full", "cls", cfg=cfg, seed=1)
    B = 2000
    images_u8 = (torch.rand(B, 3, 96, 96, generator=torch.Generator().manual_seed(4)) * 255).to(torch.uint8)
    labels = (torch.arange(B) % 10)
    # separable classes: brighten one channel stripe per class
    for c in range(10):
        rows = labels == c
        images_u8[rows, c % 3, (c * 9):(c * 9 + 9)] = 255
    images, lab = images_u8.to(dev), labels.to(dev)
    logits = torch.empty(B, 10, device=dev)
    mod.loss_and_grads(images, lab, logits_out=logits)
    torch.cuda.synchronize()
    # 8 rows of the batch against the oracle on those 8 images (rows are independent of the batch)
    idx = torch.tensor([0, 1, 2, 3, 997, 1500, 1998, 1999])
    x = (images_u8[idx].float() / 255 - 0.5) / 0.5
    with torch.no_grad():
        feats = O.forward_encoder(params, cfg, x, bf16=True)
        ref = F.linear(_r(feats[:, 0], True), _r(mod.model.head.classification.weight.detach().cpu(), True), mod.model.head.classification.bias.detach().cpu())
    assert rel_err(logits.cpu()[idx], ref) < 3e-2
    g1 = (mod.model.mae.flat_grads.clone(), mod.pos_grads.clone(), mod.head_grads.clone())
    assert all(torch.isfinite(t).all() for t in g1)
    mod.loss_and_grads(images, lab)
    assert all(torch.equal(a, b) for a, b in zip(g1, (mod.model.mae.flat_grads, mod.pos_grads, mod.head_grads)))
    losses = []
    for _ in range(10):
        loss, _c = mod.fused_training_step(images, lab, lr=1e-4)
        losses.append(loss.clone())
    losses = [float(v) for v in losses]
    assert all(math.isfinite(v) for v in losses)
    assert losses[-1] < losses[0], losses


def test_cli_pretrain_finetune_evaluate(dev, tmp_path):
    import yaml
    cfg = yaml.safe_load((ROOT / "configs" / "mae.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg["pretrain"]["batch_size"] = 256
    cfg["train"]["batch_size"] = 256
    cfg["train"]["learning_rate"] = 1e-3
    cfg["train"]["warmup_epochs"] = 1
    cfg["test"]["batch_size"] = 256
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    run = lambda *a: subprocess.run([sys.executable, "-m", *a], cwd=ROOT, capture_output=True, text=True, timeout=900)  # noqa: E731
    r = run("scripts.training.pretrain_mae", "--config", str(cfg_path), "--synthetic_images", "512", "--max_epochs", "1")
    assert r.returncode == 0, r.stderr[-3000:]
    enc = tmp_path / "outputs" / "pretrain" / "mae_pretrain" / "checkpoints" / "last.ckpt"
    r = run("scripts.training.train_mae", "--config", str(cfg_path), "--encoder_ckpt", str(enc), "--synthetic_images", "2000",
            "--max_epochs", "3")
    assert r.returncode == 0, r.stderr[-3000:]
    out = tmp_path / "outputs" / "train" / "mae_finetune"
    lines = [json.loads(x) for x in (out / "logs" / "metrics.jsonl").read_text().splitlines()]
    assert len(lines) == 3 and set(lines[0]) >= {"epoch", "train_loss", "train_acc", "val_loss", "val_acc", "lr", "images_per_s"}
    assert max(x["val_acc"] for x in lines) > 0.2  # chance is 0.1 on the separable synthetic classes
    assert (out / "checkpoints" / "best.ckpt").exists() and (out / "checkpoints" / "last.ckpt").exists() and (out / "config.yaml").exists()
    pt = torch.load(out / "vit-mae.pt", map_location="cpu", weights_only=True)
    assert "head.classification.weight" in pt and "encoder.cls_token" in pt and "encoder.blocks.0.attn.qkv.weight" in pt
    ck = torch.load(out / "checkpoints" / "best.ckpt", map_location="cpu", weights_only=True)
    assert set(ck["state_dict"]) == {"model." + k for k in pt}
    assert set(ck["hyper_parameters"]) == {"model_cfg", "training_cfg", "num_classes"}
    r = run("scripts.evaluation.evaluate_classifier", "--config", str(cfg_path), "--checkpoint", str(out / "checkpoints" / "best.ckpt"),
            "--synthetic_images", "1000")
    assert r.returncode == 0, r.stderr[-3000:]
    assert "test_acc" in r.stdout
    res = json.loads((tmp_path / "outputs" / "test" / "default" / "metrics.json").read_text())
    assert res["test_acc"] > 0.2
