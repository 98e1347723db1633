"""Host side of the fine-tuning augmentation: tests/augment_ref.py against Pillow bit for bit (every op the kernel has), the
RandAugment level table, the draw (a function of its entropy; boxes inside the image and by their acceptance rules), and
the config / command-line surface.  No GPU."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import augment_ref as R

ROOT = Path(__file__).resolve().parents[1]
FACTORS = (0.1, 0.55, 1.0, 1.45, 1.9)


def images():
    """noise / narrow-range / ramp / constant at 20, 32 and 96 pixels, the 8 x 8 set (equalize: step == 0) included."""
    out = {}
    for S in (8, 20, 32, 96):
        for name, img in R.sample_images(3, S).items():
            out[f"{name}{S}"] = img
    return out


IMAGES = images()


def to_pil(a):
    from PIL import Image
    return Image.fromarray(np.ascontiguousarray(a.transpose(1, 2, 0)), "RGB")


def from_pil(im):
    return np.asarray(im).transpose(2, 0, 1)


def same(name, got, want):
    d = got.astype(np.int32) - want.astype(np.int32)
    assert not d.any(), f"{name}: {int((d != 0).sum())} elements differ from Pillow, by up to {int(np.abs(d).max())}"


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_point_and_table_ops_match_pillow(name):
    pytest.importorskip("PIL")
    from PIL import ImageOps
    a = IMAGES[name]
    im = to_pil(a)
    same("autocontrast", R.autocontrast(a), from_pil(ImageOps.autocontrast(im)))
    same("equalize", R.equalize(a), from_pil(ImageOps.equalize(im)))
    same("invert", R.invert(a), from_pil(ImageOps.invert(im)))
    for bits in range(1, 9):
        same(f"posterize {bits}", R.posterize(a, bits), from_pil(ImageOps.posterize(im, bits)))
    assert not R.posterize(a, 0).any()
    for t in (0, 26, 128, 200, 256):
        same(f"solarize {t}", R.solarize(a, t), from_pil(ImageOps.solarize(im, t)))
    for add in (0, 55, 110, 128):   # timm's solarize_add: a point table
        lut = [min(255, i + add) if i < 128 else i for i in range(256)]
        same(f"solarize_add {add}", R.solarize_add(a, add), from_pil(im.point(lut * 3)))


def test_table_edge_cases_are_reached():
    """The inputs do reach the branches they are there for."""
    const, tiny = IMAGES["const32"], IMAGES["noise8"]
    h = np.bincount(const[0].reshape(-1), minlength=256)
    assert np.array_equal(R.autocontrast_lut(h), np.arange(256)) and np.array_equal(R.equalize_lut(h), np.arange(256))   # hi <= lo, a single bin
    h = np.bincount(tiny[0].reshape(-1), minlength=256)
    assert (h > 0).sum() > 1 and (64 - h[h > 0][-1]) // 255 == 0 and np.array_equal(R.equalize_lut(h), np.arange(256))   # step == 0
    for name in ("noise20", "noise96"):   # the min(255, .) clamp: on noise the last bins overshoot (at 32 x 32 they land on 255 exactly)
        img = IMAGES[name]
        h = np.bincount(img[0].reshape(-1), minlength=256).astype(np.int64)
        step = (img[0].size - h[h > 0][-1]) // 255
        assert step > 0 and ((step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])) // step).max() > 255


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_enhance_ops_match_pillow(name):
    pytest.importorskip("PIL")
    from PIL import ImageEnhance
    a = IMAGES[name]
    im = to_pil(a)
    for f in FACTORS:
        same(f"color {f}", R.color(a, f), from_pil(ImageEnhance.Color(im).enhance(f)))
        same(f"contrast {f}", R.contrast(a, f), from_pil(ImageEnhance.Contrast(im).enhance(f)))
        same(f"brightness {f}", R.brightness(a, f), from_pil(ImageEnhance.Brightness(im).enhance(f)))
        same(f"sharpness {f}", R.sharpness(a, f), from_pil(ImageEnhance.Sharpness(im).enhance(f)))


def matrices(S):
    return [(1, 0.27, 0, 0, 1, 0), (1, 0, 0, -0.3, 1, 0), (1, 0, 0.45 * S, 0, 1, 0), (1, 0, 0, 0, 1, -0.405 * S), R.rotate_matrix(27, S),
            R.rotate_matrix(-13.5, S), R.crop_matrix(1, 2, S - 3, S - 2, False, S), R.crop_matrix(0, 0, S, S, False, S),
            R.crop_matrix(1, 0, S // 2, S - 1, True, S)]


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_affine_matches_pillow(name):
    pytest.importorskip("PIL")
    from PIL import Image
    a = IMAGES[name]
    S = a.shape[1]
    im = to_pil(a)
    for i, m in enumerate(matrices(S)):
        for mode, resample in ((R.BILINEAR, Image.BILINEAR), (R.BICUBIC, Image.BICUBIC)):
            want = from_pil(im.transform((S, S), Image.AFFINE, m, resample, fillcolor=(128, 64, 32)))
            same(f"affine {i} mode {mode}", R.affine(a, m, mode, 0x804020), want)
    for deg in (27, -13.5, 30):
        want = from_pil(im.rotate(deg, Image.BICUBIC, fillcolor=(128, 128, 128)))
        same(f"rotate {deg}", R.affine(a, R.rotate_matrix(deg, S), R.BICUBIC, 0x808080), want)


def test_identity_and_mirror_boxes():
    for name in ("noise32", "narrow20", "ramp96"):
        a = IMAGES[name]
        S = a.shape[1]
        for mode in (R.BILINEAR_ROUND, R.BICUBIC_ROUND, R.BILINEAR, R.BICUBIC):
            assert np.array_equal(R.affine(a, R.crop_matrix(0, 0, S, S, False, S), mode), a)
            assert np.array_equal(R.affine(a, R.crop_matrix(0, 0, S, S, True, S), mode), a[:, :, ::-1])


def test_reference_and_package_agree_on_matrices_and_ids():
    from ssrl_vit_mae_jepa_amd import _lib as L
    from ssrl_vit_mae_jepa_amd import data as D
    assert (L.AUG_NONE, L.AUG_AUTOCONTRAST, L.AUG_EQUALIZE, L.AUG_INVERT, L.AUG_POSTERIZE, L.AUG_SOLARIZE, L.AUG_SOLARIZE_ADD, L.AUG_COLOR,
            L.AUG_CONTRAST, L.AUG_BRIGHTNESS, L.AUG_SHARPNESS, L.AUG_AFFINE) == tuple(range(12)) == (
        R.NONE, R.AUTOCONTRAST, R.EQUALIZE, R.INVERT, R.POSTERIZE, R.SOLARIZE, R.SOLARIZE_ADD, R.COLOR, R.CONTRAST, R.BRIGHTNESS, R.SHARPNESS, R.AFFINE)
    header = (ROOT / "include" / "mae_hip.h").read_text()
    assert "enum { MAE_AUG_NONE = 0, MAE_AUG_AUTOCONTRAST, MAE_AUG_EQUALIZE, MAE_AUG_INVERT, MAE_AUG_POSTERIZE, MAE_AUG_SOLARIZE," in header
    assert "MAE_AUG_SOLARIZE_ADD, MAE_AUG_COLOR, MAE_AUG_CONTRAST, MAE_AUG_BRIGHTNESS, MAE_AUG_SHARPNESS, MAE_AUG_AFFINE }" in header
    for deg in (27.0, -13.5, 0.0, 90.0, 333.3):
        assert D.rotate_matrix(deg, 96) == R.rotate_matrix(deg, 96)
    assert D.crop_matrix(3, 4, 50, 60, True, 96) == R.crop_matrix(3, 4, 50, 60, True, 96)
    assert D.crop_matrix(3, 4, 50, 60, False, 96) == R.crop_matrix(3, 4, 50, 60, False, 96)


def test_level_table():
    """timm's level functions of the "increasing" set, pinned at levels 0, 5, 9 and 10."""
    from ssrl_vit_mae_jepa_amd import _lib as L
    from ssrl_vit_mae_jepa_amd.data import RAND_AUGMENT_OPS, affine_arg, rand_augment_op, rotate_matrix
    S = 96
    geo = affine_arg(L.AUG_BICUBIC, 128)
    assert geo == (L.AUG_BICUBIC | (0x808080 << 8)) - 2 ** 32 and geo & 0xff == L.AUG_BICUBIC and (geo >> 8) & 0xffffff == 0x808080
    assert len(RAND_AUGMENT_OPS) == 15 and len(set(RAND_AUGMENT_OPS)) == 15
    for name, code in (("AutoContrast", L.AUG_AUTOCONTRAST), ("Equalize", L.AUG_EQUALIZE), ("Invert", L.AUG_INVERT)):
        for level in (0.0, 5.0, 9.0, 10.0):
            assert rand_augment_op(name, level, True, S) == (code, 0, (0.0,) * 6)
    want = {  # level -> (posterize bits, solarize threshold, solarize add, factor +, factor -)
        0.0: (4, 256, 0, 1.0, 1.0), 5.0: (2, 128, 55, 1.45, 0.55), 9.0: (1, 26, 99, 1.81, 0.19), 10.0: (0, 0, 110, 1.9, 0.1)}
    for level, (bits, thr, add, fp, fm) in want.items():
        assert rand_augment_op("Posterize", level, True, S)[:2] == (L.AUG_POSTERIZE, bits)
        assert rand_augment_op("Solarize", level, False, S)[:2] == (L.AUG_SOLARIZE, thr)
        assert rand_augment_op("SolarizeAdd", level, True, S)[:2] == (L.AUG_SOLARIZE_ADD, add)
        for name, code in (("Color", L.AUG_COLOR), ("Contrast", L.AUG_CONTRAST), ("Brightness", L.AUG_BRIGHTNESS), ("Sharpness", L.AUG_SHARPNESS)):
            for positive, f in ((True, fp), (False, fm)):
                c, i, a = rand_augment_op(name, level, positive, S)
                assert (c, i) == (code, 0) and a[0] == pytest.approx(f, abs=1e-12) and a[1:] == (0.0,) * 5
        for positive, sign in ((True, 1.0), (False, -1.0)):
            sh, tr = sign * 0.03 * level, sign * 0.045 * level * S
            c, i, a = rand_augment_op("ShearX", level, positive, S)
            assert (c, i) == (L.AUG_AFFINE, geo) and a == pytest.approx((1.0, sh, 0.0, 0.0, 1.0, 0.0), abs=1e-12)
            assert rand_augment_op("ShearY", level, positive, S)[2] == pytest.approx((1.0, 0.0, 0.0, sh, 1.0, 0.0), abs=1e-12)
            assert rand_augment_op("TranslateXRel", level, positive, S)[2] == pytest.approx((1.0, 0.0, tr, 0.0, 1.0, 0.0), abs=1e-9)
            assert rand_augment_op("TranslateYRel", level, positive, S)[2] == pytest.approx((1.0, 0.0, 0.0, 0.0, 1.0, tr), abs=1e-9)
            c, i, a = rand_augment_op("Rotate", level, positive, S)
            assert (c, i) == (L.AUG_AFFINE, geo) and a == rotate_matrix(sign * 3.0 * level, S)
    assert rand_augment_op("Color", 10.0, False, S)[2][0] == pytest.approx(0.1)   # the max(0.1, .) floor
    with pytest.raises(ValueError):
        rand_augment_op("Cutout", 5.0, True, S)


def test_draw_is_a_function_of_its_entropy():
    from ssrl_vit_mae_jepa_amd.data import draw_finetune_augment
    a = draw_finetune_augment(64, 96, (73, 2, 5))
    b = draw_finetune_augment(64, 96, (73, 2, 5))
    c = draw_finetune_augment(64, 96, (73, 2, 6))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a.op_codes, c.op_codes) and not torch.equal(a.crop, c.crop)
    assert a.op_codes.shape == (64, 3, 2) and a.op_codes.dtype == torch.int32
    assert a.op_args.shape == (64, 3, 6) and a.op_args.dtype == torch.float64
    assert a.erase.shape == (64, 5) and a.erase.dtype == torch.int32 and a.crop.shape == (64, 5)
    d = draw_finetune_augment(64, 96, np.random.default_rng((73, 2, 5)))
    assert torch.equal(a.op_args, d.op_args)


def test_draw_boxes_follow_their_rules():
    from ssrl_vit_mae_jepa_amd import _lib as L
    from ssrl_vit_mae_jepa_amd.data import draw_finetune_augment
    B, S = 4000, 96
    p = draw_finetune_augment(B, S, 11)
    top, left, h, w, flip = (p.crop[:, i].numpy().astype(np.int64) for i in range(5))
    assert (h > 0).all() and (w > 0).all() and (top >= 0).all() and (left >= 0).all() and (top + h <= S).all() and (left + w <= S).all()
    area, ratio = h * w / float(S * S), w / h
    whole = (h == S) & (w == S)
    # area within the scale range and aspect within the ratio range, up to the rounding of the two edges to integers
    assert (area[~whole] <= 1.0).all() and (area[~whole] >= 0.08 - 2.0 / S).all()
    assert (ratio[~whole] >= 0.75 / 1.1).all() and (ratio[~whole] <= 4.0 / 3.0 * 1.1).all()
    assert 0.45 < flip.mean() < 0.55
    codes, args = p.op_codes.numpy(), p.op_args.numpy()
    for b in range(0, B, 97):   # slot 0 is the box's matrix, in the crop's rounding mode
        moved = bool(flip[b]) or not whole[b]
        assert codes[b, 0, 0] == (L.AUG_AFFINE if moved else L.AUG_NONE)
        if moved:
            assert codes[b, 0, 1] & 0xff == L.AUG_BICUBIC_ROUND
            sx = w[b] / S
            want = (-sx, 0.0, float(left[b] + w[b]), 0.0, h[b] / S, float(top[b])) if flip[b] else (sx, 0.0, float(left[b]), 0.0, h[b] / S, float(top[b]))
            assert tuple(args[b, 0]) == want
    assert (draw_finetune_augment(50, S, 3, interpolation="bilinear").op_codes[:, 0, 1].numpy() & 0xff).max() == L.AUG_BILINEAR_ROUND
    # RandAugment slots: about half applied, every op of the list drawn, each entry one row of the level table
    ids = codes[:, 1:, 0]
    assert 0.47 < (ids != L.AUG_NONE).mean() < 0.53   # p = 0.5 over 8000 slots: five standard deviations
    assert set(np.unique(ids)) == set(range(12))
    iarg = codes[:, 1:, 1]
    geo = iarg[ids == L.AUG_AFFINE]
    assert (geo & 0xff == L.AUG_BICUBIC).all() and ((geo >> 8) & 0xffffff == 0x808080).all()
    for code, lo, hi in ((L.AUG_POSTERIZE, 0, 4), (L.AUG_SOLARIZE, 0, 256), (L.AUG_SOLARIZE_ADD, 0, 110)):
        v = iarg[ids == code]
        assert v.size and v.min() >= lo and v.max() <= hi
    f = args[:, 1:, 0][np.isin(ids, (L.AUG_COLOR, L.AUG_CONTRAST, L.AUG_BRIGHTNESS, L.AUG_SHARPNESS))]
    assert (f >= 0.1).all() and (f <= 1.9).all() and (f < 1).any() and (f > 1).any()
    # erase boxes
    e = p.erase.numpy().astype(np.int64)
    eh, ew = e[:, 1] - e[:, 0], e[:, 3] - e[:, 2]
    on = (eh > 0) & (ew > 0)
    assert 0.2 < on.mean() < 0.3
    assert ((eh == 0) & (ew == 0) & (e[:, 4] == 0))[~on].all()
    assert (e[on, 0] >= 0).all() and (e[on, 2] >= 0).all() and (e[on, 1] <= S).all() and (e[on, 3] <= S).all()
    assert (eh[on] < S).all() and (ew[on] < S).all()
    ea = eh[on] * ew[on] / float(S * S)
    assert (ea >= 0.02 * 0.8).all() and (ea <= 1.0 / 3.0 * 1.1).all()
    assert (eh[on] / ew[on] >= 0.3 / 1.2).all() and (eh[on] / ew[on] <= 1.2 / 0.3).all()
    assert len(set(e[on, 4].tolist())) > 0.99 * on.sum()


def test_probability_zero_everywhere_is_the_identity():
    from ssrl_vit_mae_jepa_amd import _lib as L
    from ssrl_vit_mae_jepa_amd.data import draw_finetune_augment
    p = draw_finetune_augment(100, 96, 5, crop_scale=None, flip=0.0, op_prob=0.0, erase_prob=0.0)
    assert (p.op_codes == L.AUG_NONE).all() and (p.op_args == 0).all() and p.erase is None
    assert torch.equal(p.crop, torch.tensor([0, 0, 96, 96, 0], dtype=torch.int32).repeat(100, 1))
    with pytest.raises(ValueError):
        draw_finetune_augment(4, 96, 5, interpolation="lanczos")
    with pytest.raises(ValueError):
        draw_finetune_augment(4, 96, 5, num_ops=8)
    with pytest.raises(ValueError):
        draw_finetune_augment(4, 96, 5, erase_prob=1.5)


def test_noise_reference_is_standard_normal_and_seeded():
    n = R.erase_noise(3, 96, 12345)
    assert abs(n.mean()) < 0.02 and abs(n.std() - 1.0) < 0.02 and np.abs(n).max() <= 5.77
    assert np.array_equal(n, R.erase_noise(3, 96, 12345)) and not np.array_equal(n, R.erase_noise(3, 96, 12346))
    assert np.array_equal(R.erase_noise(3, 96, -1), R.erase_noise(3, 96, 0xffffffff))   # the seed is the int32's bits


def test_config_and_module_options():
    import yaml
    from ssrl_vit_mae_jepa_amd.classifier import parse_augment
    base = yaml.safe_load((ROOT / "configs" / "vits8_dec192_finetune.yaml").read_text())
    aug = yaml.safe_load((ROOT / "configs" / "vits8_dec192_finetune_aug.yaml").read_text())
    block = aug["train"].pop("augment")
    assert aug == base   # the finetune config plus the block
    opts = parse_augment(block)
    assert opts == dict(crop_scale=(0.08, 1.0), flip=0.5, interpolation="bicubic", num_ops=2, magnitude=9.0, mstd=0.5, op_prob=0.5,
                        erase_prob=0.25, fill=(128, 128, 128))
    assert parse_augment(None) is None and parse_augment({}) is None
    assert parse_augment({"random_erasing": 0.1})["erase_prob"] == 0.1 and parse_augment({"random_erasing": 0.1})["crop_scale"] is None
    for bad in ({"crop_scale": [0.5]}, {"crop_scale": [0.0, 1.0]}, {"flip": 2}, {"interpolation": "nearest"}, {"rand_augment": {"num_ops": 9}},
                {"rand_augment": {"magnitude": 11}}, {"random_erasing": -0.1}, {"fill": 300}, {"colour": 1}, {"rand_augment": {"n": 2}}):
        with pytest.raises(ValueError):
            parse_augment(bad)


def test_cli_flags_parse():
    from scripts.training.train_mae import augment_overrides, build_parser
    ns = build_parser().parse_args(["--config", "c.yaml"])
    assert augment_overrides(ns, None) is None
    ns = build_parser().parse_args(["--config", "c.yaml", "--augment"])
    assert augment_overrides(ns, None) == {"crop_scale": [0.08, 1.0], "flip": 0.5, "interpolation": "bicubic",
                                           "rand_augment": {"num_ops": 2, "magnitude": 9.0, "mstd": 0.5, "prob": 0.5}, "random_erasing": 0.25,
                                           "fill": 128}
    ns = build_parser().parse_args(["--config", "c.yaml", "--crop_scale", "0.2", "1.0", "--rand_augment", "3", "7", "--random_erasing", "0.1"])
    got = augment_overrides(ns, {"flip": 0.5, "rand_augment": {"mstd": 0.25}})
    assert got == {"flip": 0.5, "crop_scale": [0.2, 1.0], "rand_augment": {"mstd": 0.25, "num_ops": 3, "magnitude": 7.0}, "random_erasing": 0.1}
