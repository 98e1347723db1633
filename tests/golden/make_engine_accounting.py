#!/usr/bin/env python3
"""Generates tests/golden/engine_accounting.json: what the engine's timers report (launches, flops, bytes per kernel class)
for every entry point on one tiny geometry.  bench.py builds its roofline from these numbers, so they are pinned: the
fixture was written on an MI355X by the commit BEFORE the engine's launch helpers were refactored, and
tests/test_gpu_engine_accounting.py requires exact equality with it (every value is a sum of integers far below 2^53,
so it is exact whatever the order of addition).  Milliseconds are never recorded.

``CASES`` maps a case name to ``setup(dev) -> (engine, run)``; ``run()`` makes the timed calls and returns the tensors
they produced (the test ignores them; an A/B of two builds of the library can compare them bit for bit).
mae_engine_decoder_decode is left out on purpose: its two LayerNorm launches were untimed before the refactor.
Needs the GPU.  Run from the repo root:
    python tests/golden/make_engine_accounting.py
"""
import ctypes as C
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd._lib import check, lib, ptr  # noqa: E402
from ssrl_vit_mae_jepa_amd.mae import MaskedAutoencoder  # noqa: E402

FIXTURE = Path(__file__).with_name("engine_accounting.json")
B, IMG, PATCH, L, NUM_CLASSES = 2, 16, 4, 17, 10
ENC = dict(embed_dim=32, depth=2, num_heads=2)
DEC = dict(decoder_embed_dim=32, decoder_depth=1, decoder_num_heads=2)
ADAM = (1e-3, 0.9, 0.999, 1e-8, 0.05)  # lr, beta1, beta2, eps, weight decay


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _model(dev, precision="bf16", **general):
    torch.manual_seed(73)
    return MaskedAutoencoder(dict(image_size=IMG, patch_size=PATCH, in_chans=3, mask_ratio=0.75, engine_precision=precision, **general),
                             ENC, DEC).to(dev)


def _images(dev, uint8=False):
    g = torch.Generator().manual_seed(74)
    x = torch.rand(B, 3, IMG, IMG, generator=g)
    return (x * 255).to(torch.uint8).to(dev) if uint8 else (x * 2 - 1).to(dev)


def _noise(dev):
    return torch.rand(B, L, generator=torch.Generator().manual_seed(75)).to(dev)


def _step(precision="bf16", uint8=False, phased=False, **general):
    def setup(dev):
        model, images, noise = _model(dev, precision, **general), _images(dev, uint8), _noise(dev)
        events = None
        if phased:  # an event in EVERY ready slot: reach_point flushes the deferred LayerNorm reductions at each point
            events = [torch.cuda.Event() for _ in model.grad_ready_points()]
            for ev in events:
                ev.record(torch.cuda.current_stream(dev))  # torch creates the HIP event lazily: force it now

        def run():
            loss, keep, mask = model.loss_and_grads(images, noise, return_indices=True, ready_events=events)
            return dict(loss=loss, keep=keep, mask=mask, grads=model.flat_grads)
        return model.engine, run
    return setup


def _forward_backward(dev):
    model, images = _model(dev), _images(dev)
    keep, mask = model.random_token_mask(B, _noise(dev))

    def run():
        x_enc = model._run_encoder(images, keep)  # mae_engine_forward_encoder with the fp32 x_encoded output
        x_pred, target = model._run_forward(images, keep, mask)  # forward_encoder + forward_decoder
        d_pred = ((2.0 / x_pred.numel()) * (x_pred - target)).contiguous()
        grads = model._run_backward(d_pred, B, keep.shape[1], mask.shape[1])  # mae_engine_backward
        return dict(x_enc=x_enc, x_pred=x_pred, **{f"grad{i}": g for i, g in enumerate(grads)})
    return model.engine, run


def _backward_halves(dev):
    model, images = _model(dev), _images(dev)
    keep, mask = model.random_token_mask(B, _noise(dev))
    k, m = keep.shape[1], mask.shape[1]
    x_pred, target = model._run_forward(images, keep, mask)  # untimed: the saved activations
    d_pred = ((2.0 / x_pred.numel()) * (x_pred - target)).contiguous()
    ws, h = model._ws(B, k, keep=True), model.engine.handle

    def run():
        gdec, genc = (torch.zeros(model.engine.trainable_elems, device=dev) for _ in range(2))
        dx = torch.empty(B, k, ENC["embed_dim"], device=dev)
        check(lib.mae_engine_backward_decoder(h, ptr(model.flat_params), ptr(model._weights()), ptr(d_pred), B, k, m, ptr(ws), ws.numel(),
                                              ptr(gdec), ptr(dx), _stream(dev)))
        check(lib.mae_engine_backward_encoder(h, ptr(model.flat_params), ptr(model._weights()), ptr(dx), B, k, ptr(ws), ws.numel(),
                                              ptr(genc), _stream(dev)))
        return dict(gdec=gdec, dx=dx, genc=genc)
    return model.engine, run


def _reconstruct(dev):
    model, images, noise = _model(dev), _images(dev), _noise(dev)

    def run():
        r = model.reconstruct(images, noise=noise)
        return dict(masked=r.masked, recon=r.reconstructed, x_pred=r.x_pred, sum_sq=r.sum_sq, sum_abs=r.sum_abs)
    return model.engine, run


def _features(with_cls):
    def setup(dev):
        model, images = _model(dev), _images(dev)
        return model.engine, lambda: dict(feats=model.extract_features(images, pool="cls" if with_cls else "mean", normalize="l2",
                                                                       with_cls=bool(with_cls)))
    return setup


def _classifier(pool, train_blocks=None, train_embed=0):
    """train_blocks None = mae_engine_classifier_forward, else mae_engine_classifier_loss_and_grads in that mode."""
    def setup(dev):
        model, images = _model(dev), _images(dev)
        D, h = ENC["embed_dim"], model.engine.handle
        head = (torch.randn(NUM_CLASSES * D + NUM_CLASSES, generator=torch.Generator().manual_seed(76)) * 0.05).to(dev)
        labels = torch.tensor([3, 7], dtype=torch.int64, device=dev)
        ws = torch.empty(lib.mae_engine_classifier_workspace_bytes(h, B, NUM_CLASSES), dtype=torch.uint8, device=dev)
        tb = ENC["depth"] if train_blocks == "depth" else train_blocks

        def run():
            out = dict(logits=torch.empty(B, NUM_CLASSES, device=dev), loss=torch.empty(1, device=dev),
                       correct=torch.empty(1, dtype=torch.int32, device=dev))
            common = [h, ptr(model.flat_params), ptr(model._weights()), ptr(head), ptr(images), _lib.MAE_F32, ptr(labels), B, pool, NUM_CLASSES]
            tail = [ptr(out["logits"]), ptr(out["loss"]), ptr(out["correct"]), _stream(dev)]
            if tb is None:
                check(lib.mae_engine_classifier_forward(*common, ptr(ws), ws.numel(), *tail))
                return out
            out.update(grads=torch.zeros(model.engine.trainable_elems, device=dev), head_grads=torch.zeros_like(head),
                       pos_grad=torch.zeros(L * D, device=dev))
            check(lib.mae_engine_classifier_loss_and_grads(*common, tb, train_embed, 1.0, ptr(ws), ws.numel(), ptr(out["grads"]),
                                                           ptr(out["head_grads"]), ptr(out["pos_grad"]), *tail))
            return out
        return model.engine, run
    return setup


def _jepa(targets_only):
    """pred_dim = embed_dim; 6 context tokens, 2 blocks of 3 targets."""
    def setup(dev):
        from ssrl_vit_mae_jepa_amd.jepa import IJEPA
        torch.manual_seed(73)
        model = IJEPA(dict(image_size=IMG, patch_size=PATCH, in_chans=3, engine_precision="bf16"), ENC,
                      dict(pred_embed_dim=32, pred_depth=1, pred_num_heads=2)).to(dev)
        model.target_arena.mul_(1.01)  # a target encoder that is not the context encoder
        images = _images(dev)
        ctx = torch.tensor([[1, 2, 5, 6, 9, 10], [3, 4, 7, 8, 11, 12]], dtype=torch.int64, device=dev)
        tgt = torch.tensor([[[13, 14, 15], [4, 8, 12]], [[1, 5, 9], [14, 15, 16]]], dtype=torch.int64, device=dev)
        net, D = model.net, ENC["embed_dim"]
        ws = model._ws(B, 6, 2, 3)

        def run():
            out = dict(loss=torch.zeros(1, device=dev), h=torch.empty(B, 2, 3, D, device=dev))
            if not targets_only:
                out.update(pred=torch.empty(B, 2, 3, D, device=dev), grads=net.flat_grads)
            check(lib.mae_engine_jepa_loss_and_grads(
                net.engine.handle, ptr(net.flat_params), ptr(net._weights()), ptr(model.target_arena), ptr(model._target_weights()),
                ptr(images), _lib.MAE_F32, ptr(ctx), ptr(tgt), B, 6, 2, 3, _lib.LOSS_MSE, 1.0, ptr(ws), ws.numel(), ptr(out.get("grads")),
                ptr(out["loss"]), ptr(out["h"]), ptr(out.get("pred")), None, 0, _stream(dev)))
            return out
        return net.engine, run
    return setup


def _optimizer(kind):
    def setup(dev):
        model = _model(dev)
        eng, T, h = model.engine, model.engine.trainable_elems, model.engine.handle
        g = torch.Generator().manual_seed(77)
        grads = (torch.randn(T, generator=g) * 0.1).to(dev)
        m, v = torch.zeros(T, device=dev), torch.zeros(T, device=dev)
        stats, scratch = torch.tensor([1.0, 1.0] + [0.0] * 6, device=dev), model._scratch_f32()
        target = model.flat_params.clone()
        target_w = torch.zeros(eng.wcache_bytes, dtype=torch.uint8, device=dev)
        params, wcache = model.flat_params, model._weights()

        def run():
            full = [h, ptr(params), ptr(grads), ptr(m), ptr(v), ptr(wcache), *ADAM, 1.0, 3, ptr(stats), ptr(scratch)]
            if kind == "optimizer_step":
                check(lib.mae_engine_optimizer_step(*full, _stream(dev)))
            elif kind == "optimizer_step_ema":
                check(lib.mae_engine_optimizer_step_ema(*full, ptr(target), ptr(target_w), 0.99, _stream(dev)))
            elif kind == "adamw_range":
                check(lib.mae_engine_adamw_range(h, ptr(params), ptr(grads), ptr(m), ptr(v), ptr(wcache), *ADAM, 3, ptr(stats), 64, T - 128,
                                                 _stream(dev)))
            else:
                check(lib.mae_engine_adamw_buffer(h, ptr(params), ptr(grads), ptr(m), ptr(v), T - 64, *ADAM, 3, ptr(stats), _stream(dev)))
            return dict(params=params, m=m, v=v, stats=stats, wcache=wcache, target=target, target_w=target_w)
        return eng, run
    return setup


CASES = {
    "loss_and_grads_bf16": _step("bf16"),
    "loss_and_grads_fp32": _step("fp32"),
    "loss_and_grads_phased": _step("bf16", phased=True),
    "loss_and_grads_uint8": _step("bf16", uint8=True),
    "loss_and_grads_norm_pix": _step("bf16", norm_pix_loss=True),
    "forward_encoder_decoder_backward": _forward_backward,
    "backward_decoder_then_encoder": _backward_halves,
    "reconstruct": _reconstruct,
    "extract_features_patches": _features(0),
    "extract_features_with_cls": _features(1),
    "classifier_forward": _classifier(_lib.POOL_CLS),
    "classifier_probe_cls": _classifier(_lib.POOL_CLS, -1, 0),
    "classifier_last1_mean": _classifier(_lib.POOL_MEAN, 1, 0),
    "classifier_full_cls_embed": _classifier(_lib.POOL_CLS, "depth", 1),
    "jepa_step": _jepa(False),
    "jepa_targets_only": _jepa(True),
    "optimizer_step": _optimizer("optimizer_step"),
    "optimizer_step_ema": _optimizer("optimizer_step_ema"),
    "adamw_range": _optimizer("adamw_range"),
    "adamw_buffer": _optimizer("adamw_buffer"),
}


def run_case(name, dev):
    """One case with timers enabled: reset, enable, run, disable, read.  Returns ({class: {launches, flops, bytes}}, outputs)."""
    eng, run = CASES[name](dev)
    eng.timers_reset()
    eng.timers_enable(True)
    try:
        outputs = run()
    finally:
        eng.timers_enable(False)
    torch.cuda.synchronize()
    acct = {}
    for cls, t in eng.timers_read().items():
        assert t["flops"] == int(t["flops"]) and t["bytes"] == int(t["bytes"]), (name, cls, t)
        acct[cls] = dict(launches=int(t["launches"]), flops=int(t["flops"]), bytes=int(t["bytes"]))
    return acct, outputs


def main():
    dev = torch.device("cuda:0")
    blob = {name: run_case(name, dev)[0] for name in CASES}
    FIXTURE.write_text(json.dumps(blob, indent=1, sort_keys=True) + "\n")
    print("wrote", FIXTURE, len(blob), "cases")


if __name__ == "__main__":
    main()
