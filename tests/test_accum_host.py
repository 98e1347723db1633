"""Gradient accumulation, host side (no GPU): the window plan of an epoch, the learning-rate scaling, the CLI flag and the
checks of ``accumulate=(index, count)``, which run before any device is asked for."""
from pathlib import Path

import pytest
import torch
import yaml

from ssrl_vit_mae_jepa_amd import IJEPAPretrainModule, MAEPretrainModule, lr_lambda
from ssrl_vit_mae_jepa_amd.data import accumulation_plan, accumulation_slots
from tests import accum_ref as R

ROOT = Path(__file__).resolve().parents[1]
GENERAL = dict(image_size=32, patch_size=8, in_chans=3, engine_precision="fp32")
ENCODER = dict(embed_dim=48, depth=2, num_heads=2)
DECODER = dict(decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)


def mae_module(**training):
    return MAEPretrainModule(dict(general=GENERAL, encoder=ENCODER, decoder=DECODER), dict(dict(batch_size=512, base_learning_rate=1.5e-4), **training))


def jepa_module(**training):
    return IJEPAPretrainModule(dict(general=GENERAL, encoder=ENCODER, predictor=dict(pred_embed_dim=32, pred_depth=1, pred_num_heads=2)),
                               dict(dict(batch_size=256, base_learning_rate=1e-3), **training))


# ---- accumulation_plan -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch,A", [(1, 1), (4, 1), (4, 3), (5, 2), (7, 8), (512, 8)])
def test_plan_counts_and_rows(batch, A):
    for n in (0, 1, batch - 1, batch, batch + 1, batch * A - 1, batch * A, batch * A + 1, 2 * batch * A + batch + 3, 3 * batch * A + 2 * batch):
        if n < 0:
            continue
        plan = accumulation_plan(n, batch, A)
        assert plan == R.plan_ref(n, batch, A), (n, batch, A)
        micro = [r for w in plan for r in w]
        assert sum(micro) == n                                                   # rows are conserved: no batch is dropped
        assert len(micro) == -(-n // batch) and len(plan) == -(-len(micro) // A)
        assert all(r == batch for r in micro[:-1]) and all(1 <= r <= batch for r in micro)
        assert all(len(w) == A for w in plan[:-1]) and all(1 <= len(w) <= A for w in plan)


def test_plan_named_cases():
    assert accumulation_plan(0, 4, 3) == []
    assert accumulation_plan(1, 4, 3) == [[1]]
    assert accumulation_plan(4, 4, 3) == [[4]]
    assert accumulation_plan(12, 4, 3) == [[4, 4, 4]]
    assert accumulation_plan(13, 4, 3) == [[4, 4, 4], [1]]
    assert accumulation_plan(22, 4, 3) == [[4, 4, 4], [4, 4, 2]]                 # a ragged tail: a short last window with a short last batch
    assert accumulation_plan(10, 4, 1) == [[4], [4], [2]]                        # A = 1: one micro-batch per window
    assert accumulation_slots([[4, 4, 4], [4, 2]]) == [(0, 3, 12, 0), (1, 3, 12, 4), (2, 3, 12, 8), (0, 2, 6, 0), (1, 2, 6, 4)]
    for bad in ((-1, 4, 1), (4, 0, 1), (4, 4, 0)):
        with pytest.raises(ValueError):
            accumulation_plan(*bad)


# ---- hyper-parameters -------------------------------------------------------------------------------------------------------
def test_effective_lr_scales_with_the_window():
    plain, acc = mae_module(), mae_module(accumulate_grad_batches=8)
    assert plain.accumulate_grad_batches == 1 and acc.accumulate_grad_batches == 8 and acc.batch_size == 512
    assert plain.effective_lr == 1.5e-4 * 512 / 256                              # without the key: the value as ever, to the bit
    assert acc.effective_lr == 1.5e-4 * 512 * 8 / 256 and acc.current_lr(0) == acc.effective_lr * lr_lambda(0, acc.warmup_epochs, acc.total_epochs)
    assert jepa_module().effective_lr == 1e-3 * 256 / 256 and jepa_module(accumulate_grad_batches=4).effective_lr == 1e-3 * 256 * 4 / 256
    with pytest.raises(ValueError):
        mae_module(accumulate_grad_batches=0)


def test_classifier_learning_rate_stays_absolute():
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule
    mc = R.micro_cfg("fp32")
    plain = ViTClassifierTrainModule(model_cfg=mc, training_cfg=dict(learning_rate=1e-3))
    acc = ViTClassifierTrainModule(model_cfg=mc, training_cfg=dict(learning_rate=1e-3, accumulate_grad_batches=4))
    assert plain.accumulate_grad_batches == 1 and acc.accumulate_grad_batches == 4
    assert acc.current_lr(0) == plain.current_lr(0)
    with pytest.raises(ValueError):
        ViTClassifierTrainModule(model_cfg=mc, training_cfg=dict(accumulate_grad_batches=0))


def test_shipped_config():
    cfg = yaml.safe_load((ROOT / "configs" / "vitb16_dec512_accum.yaml").read_text())
    base = yaml.safe_load((ROOT / "configs" / "vitb16_dec512.yaml").read_text())
    assert cfg["pretrain"]["batch_size"] * cfg["pretrain"]["accumulate_grad_batches"] == 4096 == base["pretrain"]["batch_size"]
    assert cfg["model"] == base["model"]
    mod = MAEPretrainModule.__new__(MAEPretrainModule)
    torch.nn.Module.__init__(mod)
    mod._init_training_state(cfg["pretrain"])
    ref = MAEPretrainModule.__new__(MAEPretrainModule)
    torch.nn.Module.__init__(ref)
    ref._init_training_state(base["pretrain"])
    assert mod.effective_lr == ref.effective_lr                                  # the same optimizer step as the 4096-image batch


# ---- CLI flags --------------------------------------------------------------------------------------------------------------
def test_cli_flag_overrides_the_yaml_key():
    from scripts.training import pretrain_mae, train_mae
    cfg = {"pretrain": {"batch_size": 8, "accumulate_grad_batches": 2}, "model": {"general": {}}}
    args = pretrain_mae.parse_args([])
    assert args.accumulate_grad_batches is None and pretrain_mae.apply_overrides(cfg, args)["pretrain"]["accumulate_grad_batches"] == 2
    args = pretrain_mae.parse_args(["--accumulate_grad_batches", "3"])
    out = pretrain_mae.apply_overrides(cfg, args)
    assert out["pretrain"]["accumulate_grad_batches"] == 3 and cfg["pretrain"]["accumulate_grad_batches"] == 2   # a copy
    assert out["pretrain"]["batch_size"] == 8
    # pretrain_ijepa parses with the same parser and applies the same overrides
    import inspect
    from scripts.training import pretrain_ijepa
    assert pretrain_ijepa.parse_args is pretrain_mae.parse_args and "apply_overrides(" in inspect.getsource(pretrain_ijepa.main)
    tcfg = {"train": {"batch_size": 4}}
    train_mae.apply_recipe_flags(tcfg, train_mae.parse_args([]))
    assert "accumulate_grad_batches" not in tcfg["train"]
    train_mae.apply_recipe_flags(tcfg, train_mae.parse_args(["--accumulate_grad_batches", "5"]))
    assert tcfg["train"]["accumulate_grad_batches"] == 5


def test_epoch_slots_count_optimizer_steps():
    from scripts.training.pretrain_mae import epoch_slots

    class Batches:
        n_train = 22

    mod = mae_module(batch_size=4, accumulate_grad_batches=3)
    slots, windows = epoch_slots(Batches, mod)
    assert windows == 2 and [s[:2] for s in slots] == [(0, 3), (1, 3), (2, 3), (0, 3), (1, 3), (2, 3)] and slots[-1][2:] == (10, 8)
    slots, windows = epoch_slots(Batches, mod, max_steps=1)                      # --max_steps_per_epoch counts windows and never cuts one
    assert windows == 1 and len(slots) == 3


# ---- the accumulate tuple: checked before a device is asked for ---------------------------------------------------------------
def _steps():
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule
    images, labels = torch.zeros(2, 3, 32, 32), torch.zeros(2, dtype=torch.int64)
    mae, jepa = mae_module(), jepa_module()
    clf = ViTClassifierTrainModule(model_cfg=R.micro_cfg("fp32"), training_cfg=dict(learning_rate=1e-3))
    return [
        ("mae", mae, lambda acc, rows: mae.fused_training_step(images, torch.zeros(2, 17), global_rows=rows, accumulate=acc)),
        ("ijepa", jepa, lambda acc, rows: jepa.fused_training_step(images, global_rows=rows, accumulate=acc)),
        ("classifier", clf, lambda acc, rows: clf.fused_training_step(images, labels, accumulate=acc, window_rows=rows)),
    ]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_bad_accumulate_tuples_raise_before_any_launch(which):
    name, mod, step = _steps()[which]
    for acc in ((2, 2), (3, 2), (-1, 2), (0, 0), (0, -1), (1,), "ab", (0, 1, 2)):
        with pytest.raises(ValueError):
            step(acc, 8)
    with pytest.raises(ValueError, match="row count"):                          # a window of more than one needs its rows
        step((0, 2), None)
    with pytest.raises(ValueError, match="in order"):                           # a window starts at index 0
        step((1, 2), 8)
    mod._window.advance(0, 3)                                                   # as if micro-batch 0 of 3 had been enqueued
    for acc in ((0, 3), (2, 3), (1, 2), (1, 4)):
        with pytest.raises(ValueError, match="in order"):
            step(acc, 8)
    with pytest.raises(ValueError, match="open"):                               # a plain step cannot cut into a window
        step(None, 8)
    assert (mod._window.next, mod._window.count) == (1, 3)                      # refused calls leave the window where it was
    # a well-formed tuple passes the checks and only then meets the missing device (these modules live on the host)
    with pytest.raises(RuntimeError, match="MI355X|cuda|GPU"):
        step((1, 3), 8)
    mod._window.advance(2, 3)
    with pytest.raises(RuntimeError, match="MI355X|cuda|GPU"):
        step((0, 1), None)                                                      # a window of one is the plain step: no row count needed


# ---- the inputs of tests/test_gpu_accumulate_kernel.py ------------------------------------------------------------------------
def test_kernel_inputs_meet_every_pair_of_special_values():
    import numpy as np
    d, s = R.accumulate_inputs(1024, seed=1)
    k = len(R.SPECIALS)
    seen = {(a.tobytes(), b.tobytes()) for a, b in zip(d, s)}
    assert all((a.tobytes(), b.tobytes()) in seen for a in R.SPECIALS for b in R.SPECIALS) and k * k <= 1024
    want = R.add_f32(d, s)
    assert np.isnan(want).any() and np.isinf(want).any() and (want == 0).any() and (np.abs(want[want != 0]) < R.F32_TINY).any()
