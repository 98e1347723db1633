"""Gradient accumulation through the three training modules on the GPU (-m gpu): a window of micro-batches must be the same
optimizer step as one batch of the window's rows.  The checkers are the CPU oracles on the CONCATENATED batch (never the accumulated
path itself), at the tolerances of the one-batch tests they restate (tests/test_gpu_engine.py, test_gpu_jepa.py,
test_gpu_classifier.py); MICRO models, ragged splits.  Each comparison prints its figure before it asserts."""
import numpy as np
import pytest
import torch

from oracle import jepa_oracle as J
from oracle import mae_oracle as O
from ssrl_vit_mae_jepa_amd import IJEPAPretrainModule, MAEPretrainModule
from tests import accum_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu

MICRO = R.MICRO
TCFG = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=800, warmup_epochs=20,
            batch_size=2000, base_learning_rate=1.5e-4, weight_decay=0.05)


def mae_module(dev, precision, cfg=MICRO):
    general = dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, mask_ratio=0.75, engine_precision=precision)
    module = MAEPretrainModule(dict(general=general, encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                                    decoder=dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth,
                                                 decoder_num_heads=cfg.decoder_num_heads)), TCFG)
    params = O.init_params(cfg, 73); O.randomize_params(params)
    module.model.load_state_dict(params)
    module = module.to(dev)
    module.on_train_epoch_start()
    return module, params


def window(module, images, noise, split, dev):
    """One window over ``images`` cut into micro-batches of ``split`` rows; returns the losses of all its calls."""
    rows, lo, out = sum(split), 0, []
    for i, r in enumerate(split):
        out.append(module.fused_training_step(images[lo:lo + r].to(dev), noise[lo:lo + r].contiguous().to(dev), global_rows=rows,
                                              accumulate=(i, len(split))).clone())
        lo += r
    return out


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_mae_windows_match_oracle_on_the_whole_batch(dev, precision):
    """MICRO, B = 6 as (3, 2, 1), two windows, against oracle.train_step on the 6-row batch with the same noise, at the tolerances of
    test_two_fused_steps_match_oracle: loss 1e-4 / 5e-3, gradient norm 2e-4 / 5e-2, parameters 2e-5 / 2e-2, frozen tensors bit-equal."""
    cfg, split = MICRO, (3, 2, 1)
    bf = precision == "bf16"
    module, params = mae_module(dev, precision)
    lr = O.effective_lr(1.5e-4, 2000) * O.lr_lambda(0, 20, 800)
    state = {}
    for step in (1, 2):
        images = O.synthetic_images(6, cfg, seed=100 + step)
        noise = O.make_noise(6, cfg.sequence_length, torch.Generator().manual_seed(73 + step))
        loss_ref, aux = O.train_step(params, cfg, state, images, noise, lr, step, bf16=bf)
        losses = window(module, images, noise, split, dev)
        assert module.global_step == step and module._opt_steps == step
        loss, norm = losses[-1].item(), module._stats.cpu()[0].item()
        print(f"mae {precision} window {step}: loss {loss:.8f} vs {loss_ref.item():.8f} (rel {abs(loss - loss_ref.item()) / abs(loss_ref.item()):.3e}), "
              f"grad norm rel {abs(norm - float(aux['grad_norm'])) / float(aux['grad_norm']):.3e}")
        assert abs(loss - loss_ref.item()) <= (5e-3 if bf else 1e-4) * abs(loss_ref.item())
        assert abs(norm - float(aux["grad_norm"])) <= (5e-2 if bf else 2e-4) * float(aux["grad_norm"])
        assert all(torch.isfinite(l).all() and l.item() > 0 for l in losses)
    sd = module.model.state_dict()
    worst = max((rel_err(sd[n], params[n]), n) for n in O.trainable_names(cfg))
    print(f"mae {precision}: worst parameter distance to the oracle after two windows {worst[0]:.3e} ({worst[1]})")
    for n in O.trainable_names(cfg):
        assert rel_err(sd[n], params[n]) < (2e-2 if bf else 2e-5), n
    for n in O.FROZEN + O.NO_GRAD_ON_PATH:
        assert torch.equal(sd[n].cpu(), params[n])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_window_of_one_is_the_plain_step_bit_for_bit(dev, precision):
    cfg = MICRO
    runs = []
    for acc in (None, (0, 1)):
        module, _ = mae_module(dev, precision)
        losses = []
        for step in (1, 2):
            images = O.synthetic_images(4, cfg, seed=100 + step).to(dev)
            noise = O.make_noise(4, cfg.sequence_length, torch.Generator().manual_seed(73 + step)).to(dev)
            losses.append(module.fused_training_step(images, noise, accumulate=acc).clone())
        assert module._grad_stash is None and module.global_step == 2                      # no stash for a window of one
        runs.append((module.model.flat_params.clone(), module._exp_avg.clone(), module._exp_avg_sq.clone(), torch.cat(losses), module._stats.clone()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_open_window_leaves_the_optimizer_state_alone(dev, precision):
    cfg = MICRO
    module, _ = mae_module(dev, precision)
    images = O.synthetic_images(5, cfg, seed=3).to(dev)
    noise = O.make_noise(5, cfg.sequence_length, torch.Generator().manual_seed(4)).to(dev)
    module.fused_training_step(images, noise)                                              # moments and step counters exist
    model = module.model
    before = (model.flat_params.clone(), module._exp_avg.clone(), module._exp_avg_sq.clone(), model._weights().clone())
    steps = (module.global_step, module._opt_steps)
    plain = model.loss_and_grads(images[:3].contiguous(), noise[:3].contiguous()).clone()
    own = module.fused_training_step(images[:3].contiguous(), noise[:3].contiguous(), global_rows=5, accumulate=(0, 2))
    torch.cuda.synchronize()
    assert torch.equal(own, plain)                                                         # the micro-batch's own mean loss
    assert (module.global_step, module._opt_steps) == steps
    for a, b in zip(before, (model.flat_params, module._exp_avg, module._exp_avg_sq, model._weights())):
        assert torch.equal(a, b)
    n = model.engine.trainable_elems
    assert torch.equal(module._grad_stash[:n], model.flat_grads)                           # index 0 overwrites: the stash is the weighted gradient
    assert torch.equal(module._grad_stash[n:n + 1], plain * (3 / 5.0))                     # and its loss slot the weighted loss
    with pytest.raises(ValueError):
        module.fused_training_step(images, noise)                                          # a plain step cannot cut into the window
    module.fused_training_step(images[3:].contiguous(), noise[3:].contiguous(), global_rows=5, accumulate=(1, 2))
    assert (module.global_step, module._opt_steps) == (steps[0] + 1, steps[1] + 1)
    assert not torch.equal(before[0], model.flat_params)


def test_ijepa_window_matches_oracle_on_the_whole_batch(dev):
    """fp32, one window of (3, 1) rows, masks drawn once for the 4 rows, against jepa_oracle.train_step on the 4-row batch at the
    tolerances of test_two_fused_steps_with_ema_match_oracle (loss 1e-4, gradient norm 3e-4, parameters and EMA target 3e-4)."""
    cfg, split = J.JEPA_MICRO, (3, 1)
    mc = dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision="fp32", loss="mse",
                           num_target_blocks=cfg.num_target_blocks, target_scale=cfg.target_scale, target_aspect=cfg.target_aspect,
                           context_scale=cfg.context_scale),
              encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
              predictor=dict(pred_embed_dim=cfg.pred_embed_dim, pred_depth=cfg.pred_depth, pred_num_heads=cfg.pred_num_heads))
    tcfg = dict(total_epochs=10, warmup_epochs=2, steps_per_epoch=4, batch_size=512, base_learning_rate=1.5e-4, weight_decay=0.05,
                ema_start=0.9, ema_end=1.0)
    module = IJEPAPretrainModule(mc, tcfg)
    params = J.init_params(cfg, 73); J.M.randomize_params(params)
    module.model.net.load_state_dict(params)
    module.model.reset_target()
    module = module.to(dev)
    target = {k: v.clone() for k, v in params.items()}
    lr = module.current_lr()
    images = J.M.synthetic_images(4, cfg.as_mae(), seed=101)
    ctx, tgt = J.sample_masks(cfg, 4, torch.Generator().manual_seed(1))
    mom = J.ema_momentum_at(0, 40, 0.9, 1.0)
    loss_ref, aux = J.train_step(params, target, cfg, {}, images, ctx, tgt, lr, 1, mom)
    target0 = module.model.target_arena.clone()
    lo = 0
    for i, r in enumerate(split):
        loss = module.fused_training_step(images[lo:lo + r].to(dev), ctx[lo:lo + r].contiguous(), tgt[lo:lo + r].contiguous(), global_rows=4,
                                          accumulate=(i, len(split)))
        if i == 0:
            assert module.global_step == 0 and module._opt_steps == 0 and torch.equal(module.model.target_arena, target0)   # one EMA sweep per window
        lo += r
    norm = module._stats[0].item()
    print(f"ijepa window: loss rel {abs(loss.item() - loss_ref.item()) / abs(loss_ref.item()):.3e}, grad norm rel "
          f"{abs(norm - float(aux['grad_norm'])) / float(aux['grad_norm']):.3e}")
    assert module.global_step == 1 and module._opt_steps == 1
    assert abs(loss.item() - loss_ref.item()) <= 1e-4 * abs(loss_ref.item())
    assert abs(norm - float(aux["grad_norm"])) <= 3e-4 * float(aux["grad_norm"]) and module._stats[1].item() == 1.0
    sd, tsd = module.model.net.state_dict(), module.model.target_state_dict()
    for n in J.trainable_names(cfg):
        assert rel_err(sd[n], params[n]) < 3e-4, n
    for n in J.ema_names(cfg):
        assert rel_err(tsd[n], target[n]) < 3e-4, n
        assert not torch.equal(tsd[n].cpu(), sd[n].cpu())
    for n in J.M.FROZEN:
        assert torch.equal(sd[n].cpu(), params[n])


@pytest.mark.parametrize("mode", ["full", "frozen"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_classifier_windows_match_reference_on_the_whole_batch(dev, precision, mode):
    """Hard labels, B = 6 as (4, 2), two windows, against the reference scaffolding of test_two_steps_match_reference on the 6-row batch
    at its tolerances: loss 1e-4 / 2e-2, parameters 2e-5 / 2e-2 (the key third of attn.qkv.bias left out: its exact gradient is zero),
    the pos_embed displacement within 1e-3 / 1.5e-1; ``correct`` is the sum over the micro-batches."""
    cfg, split, lr, pool = MICRO, (4, 2), 1e-3, "cls"
    bf = precision == "bf16"
    mod, params = R.build_classifier(dev, precision, mode, pool)
    names = R.trainable_names(mod)
    p = R.ref_step_state(mod, params)
    p0 = {k: v.clone() for k, v in p.items()}
    state = {}
    g = torch.Generator().manual_seed(11)
    for step in (1, 2):
        images = O.synthetic_images(6, cfg, seed=20 + step)
        labels = torch.randint(0, 10, (6,), generator=g)
        # each micro-batch's own count, from plain native calls with the weights the window will see
        own = [int(mod.loss_and_grads(images[a:b].to(dev), labels[a:b].to(dev))[1].item()) for a, b in ((0, 4), (4, 6))]
        l0, c0 = mod.fused_training_step(images[:4].to(dev), labels[:4].to(dev), lr=lr, accumulate=(0, 2), window_rows=6)
        assert int(c0.item()) == own[0] and mod._opt_steps == step - 1
        loss, correct = mod.fused_training_step(images[4:].to(dev), labels[4:].to(dev), lr=lr, accumulate=(1, 2), window_rows=6)
        torch.cuda.synchronize()
        assert mod._opt_steps == step and int(correct.item()) == sum(own)
        assert abs(float(mod.logged["train_acc"]) - sum(own) / 6.0) < 1e-6 and float(mod.logged["train_loss"]) == float(loss)
        lref, gref, _ = R.ref_loss_and_grads(p, cfg, images, labels, names, pool, bf)
        print(f"classifier {precision} {mode} window {step}: loss {float(loss):.8f} vs {float(lref):.8f}")
        assert abs(float(loss) - float(lref)) <= (2e-2 if bf else 1e-4) * abs(float(lref)), (step, float(loss), float(lref))
        gn = R.native_grads(mod)                                                           # the live buffers hold the window's gradient
        for n in names:
            assert rel_err(gn[n], gref[n]) < (5e-2 if bf else 2e-4), (step, n, rel_err(gn[n], gref[n]))
        gref = {k: v.clone() for k, v in gref.items()}
        O.clip_grad_norm(gref, 1.0)
        pp = {k: p[k] for k in names}
        O.adamw_step(pp, gref, state, lr, step, weight_decay=0.05)
        p.update(pp)
    sd = {k: v.detach().cpu().double() for k, v in mod.model.state_dict().items()}
    tp, D = (2e-2 if bf else 2e-5), cfg.embed_dim
    for n in names:
        a, b = sd[n], p[n]
        if n.endswith("attn.qkv.bias"):
            a, b = torch.cat([a[:D], a[2 * D:]]), torch.cat([b[:D], b[2 * D:]])
        assert rel_err(a, b) < tp, (n, rel_err(a, b))
        assert not torch.equal(sd[n], p0[n]), n
    for n in sd:
        if n not in names and n in p0:
            assert torch.equal(sd[n], p0[n]), n                                            # frozen tensors keep their bits
    if mode == "full":
        q0 = params["encoder.vit.pos_embed"].double()
        assert float((sd["encoder.pos_embed"] - q0).abs().max()) > 1e-4
        assert rel_err(sd["encoder.pos_embed"] - q0, p["encoder.pos_embed"] - q0) < (1.5e-1 if bf else 1e-3)


def test_classifier_soft_targets_and_drop_path_sum_per_micro_batch(dev):
    """Mixup / CutMix + label smoothing + a drop-path table, one window of (4, 2): the gradient the optimizer reads equals the sum of the
    two micro-batches' gradients from separate ``loss_and_grads`` calls with the same draws and weights, added in fp64 on the host, within
    2 fp32 ulps of the larger addend per element (the window performs ONE fp32 add per element: half an ulp of the sum)."""
    from ssrl_vit_mae_jepa_amd.data import draw_drop_path, draw_mix_params, mix_batch
    cfg, split = MICRO, (4, 2)
    tc = dict(label_smoothing=0.1, mixup_alpha=0.8, cutmix_alpha=1.0, drop_path=0.2)
    mod, _ = R.build_classifier(dev, "fp32", "full", training_cfg=tc)
    images = (torch.rand(6, 3, 32, 32, generator=torch.Generator().manual_seed(8)) * 255).to(torch.uint8).to(dev)
    labels = torch.randint(0, 10, (6,), generator=torch.Generator().manual_seed(9)).to(dev)
    depth = len(mod.model.encoder.blocks)
    parts, lo = [], 0
    for i, r in enumerate(split):                                                        # the draws of steps 0 and 1, as the module makes them
        x, y = images[lo:lo + r].contiguous(), labels[lo:lo + r].contiguous()
        scale = draw_drop_path(depth, r, mod.drop_path, (mod.drop_seed, mod.current_epoch, i))
        mp = draw_mix_params(r, x.shape[-1], (mod.mix_seed, mod.current_epoch, i), mod.mixup_alpha, mod.cutmix_alpha, mod.mix_prob, mod.mix_switch_prob)
        xm, ya, yb, lam = mix_batch(x, y, mp)
        mod.loss_and_grads(xm, ya, grad_scale=r / 6.0, labels_b=yb, lam=lam, branch_scale=scale)
        torch.cuda.synchronize()
        parts.append(R.native_grads(mod))
        lo += r
    assert (mod._mix_step, mod._drop_step) == (0, 0)
    lo = 0
    for i, r in enumerate(split):
        mod.fused_training_step(images[lo:lo + r].contiguous(), labels[lo:lo + r].contiguous(), lr=1e-3, accumulate=(i, 2), window_rows=6)
        lo += r
    torch.cuda.synchronize()
    assert (mod._mix_step, mod._drop_step, mod._opt_steps) == (2, 2, 1)                  # draws per micro-batch, one optimizer step
    got = R.native_grads(mod)
    worst = 0.0
    for n, gw in got.items():
        a, b = parts[0][n].numpy(), parts[1][n].numpy()
        assert np.isfinite(gw.numpy()).all() and np.abs(gw.numpy()).max() > 0, n
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32)).astype(np.float64)
        err = np.abs(gw.numpy() - (a + b)) / ulp
        worst = max(worst, float(err.max()))
        assert float(err.max()) <= 2.0, (n, float(err.max()))
    print(f"classifier soft targets + drop path: worst |window - (a + b)| = {worst:.3f} ulp of the larger addend")
