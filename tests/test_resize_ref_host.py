"""The resize reference of tests/resize_ref.py on the host: it is torch's antialiased bilinear interpolation for whole-image
boxes, the identity and the mirror where it must be, the kernel's fp32 arithmetic stays inside the derived bound on every case
of the table, and the loaders / wrapper / C ABI carry the new step without changing the 96 px path."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import resize_ref as R

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("Si,So", [(96, 112), (96, 224), (32, 64), (96, 32), (96, 40), (96, 12), (12, 7), (8, 18), (8, 21), (96, 96)])
def test_reference_is_torch_antialiased_bilinear(Si, So):
    g = np.random.default_rng(Si * 1000 + So)
    x = g.standard_normal((2, 3, Si, Si))
    ref, _ = R.resize_reference(x.astype(np.float32), None, So)
    x32 = x.astype(np.float32).astype(np.float64)
    want = F.interpolate(torch.from_numpy(x32), size=(So, So), mode="bilinear", antialias=True, align_corners=False).numpy()
    err = float(np.abs(ref - want).max())
    print(f"{Si} -> {So}: worst |reference - F.interpolate| {err:.3e} (bound 1e-9)")
    assert err <= 1e-9


def test_identity_and_flip():
    u8, f32 = R.inputs(4, 3, 96)
    for x in (u8, f32):
        ref, delta = R.resize_reference(x, R.whole(4, 96), 96)
        assert np.array_equal(ref, x.astype(np.float64))
        ref, _ = R.resize_reference(x, R.whole(4, 96, 1), 96)
        assert np.array_equal(ref, x.astype(np.float64)[..., ::-1])
        assert np.array_equal(R.resize_emulated_f32(x, R.whole(4, 96), 96), x.astype(np.float32))       # the kernel's arithmetic copies too
        assert np.array_equal(R.resize_emulated_f32(x, R.whole(4, 96, 1), 96), x.astype(np.float32)[..., ::-1])
    assert np.array_equal(R.resize_reference(u8, None, 96)[0], R.resize_reference(u8, R.whole(4, 96), 96)[0])


@pytest.mark.parametrize("case", R.CASES + [(1, 1, 96, 12)], ids=lambda c: "x".join(map(str, c)))
def test_fp32_emulation_stays_inside_delta(case):
    B, C, Si, So = case
    u8, f32 = R.inputs(B, C, Si)
    for name, params in R.box_sets(B, Si):
        for kind, x in (("u8", u8), ("f32", f32)):
            ref, delta = R.reference(case, name, params, kind)
            emu = R.resize_emulated_f32(x, params, So).astype(np.float64)
            ratio = float((np.abs(emu - ref) / delta).max())
            print(f"{case} {name} {kind}: worst |fp32 - fp64| {float(np.abs(emu - ref).max()):.3e}, delta <= {float(delta.max()):.3e}, worst ratio {ratio:.3f}")
            assert ratio <= 1.0
            if kind == "u8":
                assert 1e-4 < float(delta.min()) and float(delta.max()) < 1e-2   # above what fp32 reaches, below the old crop test's allowance
                assert float(np.abs(R.round_u8(emu).astype(np.float64) - ref).max()) <= 0.5 + float(delta.max())


def test_box_sets_are_valid_boxes():
    from ssrl_vit_mae_jepa_amd.data import check_boxes
    for B, C, Si, So in R.CASES:
        sets = R.box_sets(B, Si)
        assert {n for n, _ in sets} >= {"whole", "flip", "1x1", "borders0", "column", "row", "rrc08", "rrc80"}
        for _name, p in sets:
            assert p.shape == (B, 5) and p.dtype == np.int32
            check_boxes(torch.from_numpy(p), Si)


def test_bad_boxes_and_bad_batches_raise():
    from ssrl_vit_mae_jepa_amd.data import check_boxes, resize_batch
    good = torch.tensor([[0, 0, 96, 96, 0], [95, 95, 1, 1, 1]])
    check_boxes(good, 96)
    for bad in ([-1, 0, 10, 10, 0], [0, -1, 10, 10, 0], [0, 0, 0, 10, 0], [0, 0, 10, 0, 1], [90, 0, 7, 10, 0], [0, 90, 10, 7, 0], [0, 0, 97, 96, 0]):
        with pytest.raises(ValueError, match="does not lie inside"):
            check_boxes(torch.tensor([good[0].tolist(), bad]), 96)
    with pytest.raises(ValueError):
        check_boxes(torch.zeros(3, 4, dtype=torch.int64), 96)
    with pytest.raises(ValueError, match="CUDA"):  # no CPU fallback: a host batch is refused, loudly
        resize_batch(torch.zeros(1, 3, 96, 96, dtype=torch.uint8), 112)


def test_loaders_keep_the_dataset_path():
    """A 96 px or model-less configuration is served as before: the stored uint8 batches, no resize step."""
    from ssrl_vit_mae_jepa_amd import data as D
    cpu = torch.device("cpu")
    for cfg in ({"train": {"batch_size": 8, "samples_per_class": 4}, "test": {"batch_size": 8}},
                {"train": {"batch_size": 8, "samples_per_class": 4}, "model": {"general": {"image_size": 96, "patch_size": 8}}}):
        assert D.model_image_size(cfg) == 96 and D.labeled_serving(cfg) == (None, None)
        train_b, val_b = D.get_train_batches(cfg, cpu, synthetic_images=100)
        test_b = D.get_test_batches(cfg, cpu, synthetic_images=40)
        for loader in (train_b, val_b, test_b):
            assert loader.image_size is None
            x, y = next(iter(loader()))
            assert x.dtype == torch.uint8 and tuple(x.shape[1:]) == (3, 96, 96) and y.dtype == torch.int64
        imgs, _ = D.synthetic_labeled(100, seed=73)
        assert torch.equal(next(iter(val_b()))[0], imgs[val_b.idx[:8]])
    big = {"train": {"batch_size": 8}, "model": {"general": {"image_size": 224, "patch_size": 16}}}
    assert D.labeled_serving(big) == (224, torch.uint8)
    assert D.labeled_serving({"model": {"general": {"image_size": 224, "patch_size": 14}}}) == (224, torch.float32)
    train_b, val_b = D.get_train_batches(big, cpu, synthetic_images=100, train_at_dataset_size=True)
    assert train_b.image_size is None and val_b.image_size == 224
    with pytest.raises(ValueError, match="CUDA"):   # the resize has no host path
        next(iter(val_b()))
    # the pretraining loader at 96 px on the host: the old path, float synthetic images as before
    pre = {"pretrain": {"batch_size": 4, "val_split": 0.25}, "engine": {"data_on_device": True}}
    tb, vb = D.get_pretrain_batches(pre, cpu, synthetic_images=8)
    sb = next(iter(tb(0)))
    assert tuple(sb.images.shape) == (4, 3, 96, 96) and sb.images.dtype == torch.float32


def test_header_and_binding_carry_the_symbol():
    from ssrl_vit_mae_jepa_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "mae_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+mae_resize_crop_flip\s*\(([^)]*)\)", header)
    assert m, "mae_resize_crop_flip is not declared in include/mae_hip.h"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10 and args[0].startswith("const void*") and args[5].startswith("const int32_t*") and args[-1].startswith("void*")
    res, argtypes = _lib.SIGNATURES["mae_resize_crop_flip"]
    assert len(argtypes) == 10 and hasattr(_lib.lib, "mae_resize_crop_flip")
    assert _lib.ABI_VERSION == 4
    # refusals need no device: they come before any launch
    assert _lib.lib.mae_resize_crop_flip(None, _lib.MAE_U8, 1, 3, 96, None, 112, _lib.MAE_U8, None, None) != 0
    assert b"null" in _lib.lib.mae_last_error()
