"""References for the gradient-accumulation tests (tests/test_accum_host.py, tests/test_gpu_accumulate_*.py): the window plan
restated without the product's code, the special values the accumulate kernel is fed, and the classifier's reference
scaffolding of tests/test_gpu_classifier.py::test_two_steps_match_reference (restated here: that file stays as it is)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mae_oracle as O

MICRO = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=2, num_heads=2,
                    decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


# ---- the window plan ---------------------------------------------------------------------------------------------------
def plan_ref(n_rows: int, batch: int, accumulate: int):
    """Row by row: a micro-batch closes at ``batch`` rows, a window at ``accumulate`` micro-batches, both at the end of the epoch."""
    windows, window, rows = [], [], 0
    for _ in range(n_rows):
        rows += 1
        if rows == batch:
            window.append(rows)
            rows = 0
            if len(window) == accumulate:
                windows.append(window)
                window = []
    if rows:
        window.append(rows)
    if window:
        windows.append(window)
    return windows


# ---- inputs of the accumulate kernel -----------------------------------------------------------------------------------
F32_MAX = np.finfo(np.float32).max
F32_TINY = np.finfo(np.float32).tiny          # smallest normal
F32_DENORM = np.float32(1e-45)                # smallest denormal
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, F32_DENORM, -F32_DENORM, F32_TINY / 2, -F32_TINY / 2, F32_TINY, F32_MAX, -F32_MAX,
                     1.0, -1.0, 1e-8, 16777216.0], dtype=np.float32)


def accumulate_inputs(n: int, seed: int):
    """(dst, src) of n floats: every pair of SPECIALS meets at least once (sums that overflow, cancel to +-0, leave the denormal
    range, inf - inf), the rest are normal values over 12 decades with both signs."""
    rng = np.random.default_rng(seed)
    mag = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), size=(2, n))).astype(np.float32)
    sign = rng.integers(0, 2, size=(2, n)).astype(np.float32) * 2 - 1
    dst, src = mag[0] * sign[0], mag[1] * sign[1]
    k = len(SPECIALS)
    pairs = min(n, k * k)
    pos = rng.permutation(n)[:pairs]              # scattered over the buffer: every part of the grid sees some
    idx = np.arange(pairs)
    dst[pos], src[pos] = SPECIALS[idx // k], SPECIALS[idx % k]
    return dst, src


def same_values(a: np.ndarray, b: np.ndarray) -> bool:
    """Bit-identical, except that NaNs compare as values (any NaN equals any NaN)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]))


def add_f32(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (dst.astype(np.float32) + src.astype(np.float32)).astype(np.float32)


# ---- classifier reference (tests/test_gpu_classifier.py, restated) -----------------------------------------------------
def _r(x, bf):
    return x.to(torch.bfloat16).to(torch.float32) if bf else x


def micro_cfg(precision, pool="cls", cfg=MICRO):
    return dict(general=dict(image_size=cfg.image_size, patch_size=cfg.patch_size, in_chans=cfg.in_chans, engine_precision=precision),
                encoder=dict(embed_dim=cfg.embed_dim, depth=cfg.depth, num_heads=cfg.num_heads),
                decoder=dict(decoder_embed_dim=cfg.decoder_embed_dim, decoder_depth=cfg.decoder_depth, decoder_num_heads=cfg.decoder_num_heads),
                head=dict(embed_dim=cfg.embed_dim, pool=pool))


def build_classifier(dev, precision, mode, pool="cls", cfg=MICRO, C=10, seed=5, training_cfg=None):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    mc = micro_cfg(precision, pool, cfg)
    mae = encoder_mae(mc)
    params = O.init_params(cfg, 73)
    O.randomize_params(params, seed=seed)
    mae.load_state_dict(params)
    torch.manual_seed(seed)
    mod = ViTClassifierTrainModule(pretrained_encoder=mae.encoder.vit, model_cfg=mc,
                                   training_cfg=dict(dict(learning_rate=1e-3, weight_decay=0.05, freeze_encoder=True), **(training_cfg or {})),
                                   num_classes=C)
    if mode == "frozen":
        mod.freeze_encoder()
    elif mode == "full":
        mod.unfreeze_encoder()
    else:
        mod.unfreeze_last_layers(int(mode[len("last"):]))
    return mod.to(dev), params


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
    """name -> gradient the native step left in the live buffers (ViTClassifier naming), fp64 on the host."""
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
    return {k: v.double().clone() for k, v in out.items()}
