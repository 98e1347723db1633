"""Models of another size than the 96 px dataset, end to end on the MI355X: the loaders resize on the device
(``data.resize_batch``) and every consumer -- the MAE and I-JEPA steps, classifier training with ``train.augment`` and mixup,
evaluation, feature extraction / k-NN, the linear probe with ``--augment crop``, the reconstruction evaluator and the pretrain
CLI -- runs a 112 px / patch 16 model (49 tokens; width 64, two heads of 32), plus one 32 px / patch 8 model behind the
downsampling path."""
import math
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
ENCODER = dict(embed_dim=64, depth=2, num_heads=2)
DECODER = dict(decoder_embed_dim=64, decoder_depth=1, decoder_num_heads=2)
PRETRAIN = dict(mask_ratio_start=0.75, mask_ratio_end=0.75, mask_ramp_epochs=5, total_epochs=2, warmup_epochs=1, batch_size=8,
                base_learning_rate=1.5e-4, weight_decay=0.05, val_split=0.5, data_fraction=1.0)


def model_cfg(size=112, patch=16, **extra):
    return dict(general=dict(image_size=size, patch_size=patch, in_chans=3), encoder=dict(ENCODER), decoder=dict(DECODER),
                head=dict(embed_dim=ENCODER["embed_dim"], pool="cls"), **extra)


def with_precision(mc, precision="bf16"):
    return dict(mc, general=dict(mc["general"], engine_precision=precision))


def full_cfg(tmp_path, size=112, patch=16, **train):
    return dict(model=model_cfg(size, patch), pretrain=dict(PRETRAIN),
                train=dict(dict(samples_per_class=6, total_epochs=2, warmup_epochs=1, batch_size=16, learning_rate=1e-3, weight_decay=0.05,
                                freeze_encoder=False), **train),
                test=dict(batch_size=16), logging=dict(output_dir_base=str(tmp_path / "outputs"), model_path="vit-mae.pt"),
                engine=dict(precision="bf16", fused_step=True, data_on_device=True), seed=73)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


@pytest.fixture()
def unlabeled_file(tmp_path, monkeypatch):
    """A 32-image stand-in for unlabeled_X.bin (uint8, planes column-major as the STL-10 file stores them)."""
    from ssrl_vit_mae_jepa_amd import data as D
    g = np.random.default_rng(11)
    imgs = g.integers(0, 256, (32, 3, 96, 96), dtype=np.uint8)
    path = tmp_path / "unlabeled_X.bin"
    np.ascontiguousarray(imgs.transpose(0, 1, 3, 2)).tofile(path)
    monkeypatch.setattr(D, "STL10_UNLABELED", path)
    return torch.from_numpy(imgs)


def test_pretrain_batches_at_model_size(dev, tmp_path, unlabeled_file):
    from ssrl_vit_mae_jepa_amd import data as D
    cfg = full_cfg(tmp_path)
    for on_device in (True, False):   # resident on the device / streamed from pinned memory
        cfg["engine"]["data_on_device"] = on_device
        train_b, val_b = D.get_pretrain_batches(cfg, dev)
        plain = D.resize_batch(unlabeled_file.to(dev), 112)
        perm = torch.randperm(32, generator=torch.Generator().manual_seed(73))
        got = [sb.images for sb in val_b()]
        torch.cuda.synchronize()
        assert [tuple(x.shape) for x in got] == [(8, 3, 112, 112)] * 2 and all(x.dtype == torch.uint8 for x in got)
        assert torch.equal(torch.cat(got), plain[perm[16:].to(dev)])   # no augmentation at data_fraction 1: the plain resize
        sb = next(iter(train_b(0)))
        assert tuple(sb.images.shape) == (8, 3, 112, 112) and sb.images.dtype == torch.uint8 and sb.global_rows == 8
    # a patch-14 geometry reads no bytes: normalised fp32, bit-identical to normalize_u8 of the uint8 resize
    cfg14 = full_cfg(tmp_path, patch=14)
    x14 = next(iter(D.get_pretrain_batches(cfg14, dev)[1]())).images
    assert x14.dtype == torch.float32 and tuple(x14.shape) == (8, 3, 112, 112)
    assert torch.equal(x14.cpu(), D.normalize_u8(got[0].cpu()))
    # the synthetic stand-in is float: resized as it is, no normalisation
    xs = next(iter(D.get_pretrain_batches(cfg, dev, synthetic_images=16)[1]())).images
    assert xs.dtype == torch.float32 and tuple(xs.shape) == (8, 3, 112, 112) and float(xs.abs().max()) <= 1.0 + 1e-6


def test_augmented_batch_is_resize_of_the_same_draw(dev, tmp_path, unlabeled_file):
    """data_fraction < 1 augments: the box is drawn at the source size by the unchanged draw_augment_params (generator seed + 7)
    and resampled to 112 px in the one resize pass."""
    from ssrl_vit_mae_jepa_amd import data as D
    cfg = full_cfg(tmp_path)
    cfg["pretrain"]["data_fraction"] = 0.5      # the first 16 images, 8 train / 8 val
    _train_b, val_b = D.get_pretrain_batches(cfg, dev)
    got = next(iter(val_b())).images
    perm = torch.randperm(16, generator=torch.Generator().manual_seed(73))
    src = unlabeled_file[:16][perm[8:]].to(dev)
    draw = D.draw_augment_params(8, 96, torch.Generator(device=dev).manual_seed(73 + 7))
    want = D.resize_batch(src, 112, params=draw)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert not torch.equal(got, D.resize_batch(src, 112))   # the draw moved something


def test_mae_and_ijepa_steps(dev, tmp_path, unlabeled_file):
    from ssrl_vit_mae_jepa_amd import data as D
    from ssrl_vit_mae_jepa_amd.jepa import IJEPAPretrainModule
    from ssrl_vit_mae_jepa_amd.training import MAEPretrainModule
    losses = {}
    for size, patch in ((112, 16), (32, 8)):   # 96 -> 112 upsamples, 96 -> 32 runs the antialiasing filter
        cfg = full_cfg(tmp_path, size, patch)
        images = next(iter(D.get_pretrain_batches(cfg, dev)[0](0))).images
        assert tuple(images.shape) == (8, 3, size, size) and images.dtype == torch.uint8
        mc = with_precision(cfg["model"])
        mae = MAEPretrainModule(dict(general=mc["general"], encoder=mc["encoder"], decoder=mc["decoder"]), PRETRAIN).to(dev)
        losses[f"mae{size}"] = mae.fused_training_step(images, lr=1e-4).clone()
    images = next(iter(D.get_pretrain_batches(full_cfg(tmp_path), dev)[0](0))).images
    mc = with_precision(model_cfg())
    jepa = IJEPAPretrainModule(dict(general=mc["general"], encoder=mc["encoder"], predictor=dict(pred_embed_dim=32, pred_depth=1, pred_num_heads=2)),
                               dict(PRETRAIN, steps_per_epoch=4)).to(dev)
    losses["ijepa112"] = jepa.fused_training_step(images, lr=1e-4).clone()
    torch.cuda.synchronize()
    print({k: float(v) for k, v in losses.items()})
    assert all(math.isfinite(float(v)) for v in losses.values()), losses


def classifier(dev, cfg):
    from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae
    mc = with_precision(cfg["model"])
    torch.manual_seed(5)
    mod = ViTClassifierTrainModule(pretrained_encoder=encoder_mae(mc).encoder.vit, model_cfg=mc, training_cfg=cfg["train"], num_classes=10)
    mod.unfreeze_encoder()
    return mod.to(dev)


AUGMENT = dict(crop_scale=[0.08, 1.0], flip=0.5, interpolation="bicubic", rand_augment=dict(num_ops=2, magnitude=9, mstd=0.5, prob=0.5))


def test_classifier_step_with_augment_and_mixup(dev, tmp_path):
    """train.augment runs on the dataset's 96 px bytes, the resize to 112 px follows (uint8 without erasing, the erased fp32
    batch with it), then mixup / CutMix at the model's size."""
    from ssrl_vit_mae_jepa_amd import data as D
    for erase in (0.25, 0.0):
        cfg = full_cfg(tmp_path, augment=dict(AUGMENT, random_erasing=erase), mixup_alpha=0.8, cutmix_alpha=1.0, label_smoothing=0.1)
        train_b, val_b = D.get_train_batches(cfg, dev, synthetic_images=100, train_at_dataset_size=True)
        mod = classifier(dev, cfg)
        imgs, labels = next(iter(train_b(0)))
        assert tuple(imgs.shape[1:]) == (3, 96, 96) and imgs.dtype == torch.uint8          # augmented where the bytes live
        aug = mod._augment(imgs)
        assert tuple(aug.shape) == (imgs.shape[0], 3, 112, 112) and aug.dtype == (torch.float32 if erase else torch.uint8)
        losses = [mod.fused_training_step(imgs, labels, lr=1e-3)[0].clone() for _ in range(2)]
        vi, vl = next(iter(val_b()))
        assert tuple(vi.shape[1:]) == (3, 112, 112) and vi.dtype == torch.uint8             # validation: the plain resize
        with torch.no_grad():
            _logits, vloss, _correct = mod.model.evaluate(vi, vl)
        torch.cuda.synchronize()
        assert all(math.isfinite(float(v)) for v in losses + [vloss]), (erase, losses, vloss)
        with pytest.raises(ValueError, match="doesn't match model"):   # without the augmentation a 96 px batch is still refused
            mod.loss_and_grads(imgs, labels)


def test_features_knn_and_reconstruction(dev, tmp_path):
    from ssrl_vit_mae_jepa_amd import data as D
    from ssrl_vit_mae_jepa_amd.mae import MaskedAutoencoder
    from ssrl_vit_mae_jepa_amd.reconstruction import evaluate_reconstruction
    from ssrl_vit_mae_jepa_amd.representation import extract_split_features, knn_classify, load_eval_encoder
    cfg = full_cfg(tmp_path)
    train_b, val_b = D.get_train_batches(cfg, dev, synthetic_images=100)
    test_b = D.get_test_batches(cfg, dev, synthetic_images=40)
    assert all(tuple(next(iter(b()))[0].shape[1:]) == (3, 112, 112) for b in (train_b, val_b, test_b))
    enc = load_eval_encoder("random", cfg["model"], precision="bf16", device=dev)
    bank_f, bank_y = extract_split_features(enc, train_b, pool="cls", normalize="l2")
    query_f, query_y = extract_split_features(enc, test_b, pool="cls", normalize="l2")
    assert tuple(bank_f.shape) == (60, 64) and tuple(query_f.shape) == (40, 64) and bool(torch.isfinite(bank_f).all())
    acc = knn_classify(bank_f, bank_y, query_f, query_y, ks=(5,), num_classes=10)
    assert 0.0 <= acc[5] <= 1.0
    mc = with_precision(cfg["model"])
    mae = MaskedAutoencoder(mc["general"], mc["encoder"], mc["decoder"]).to(dev)
    st = evaluate_reconstruction(mae, val_b, mask_ratio=0.75, mask_seed=5)
    assert st["images"] == 40 and math.isfinite(st["mse"]) and math.isfinite(st["psnr"])


def test_linear_probe_epoch_with_crop(dev, tmp_path):
    """scripts.evaluation.linear_probe, in process: cached validation / test features from the plain resize, training features
    re-extracted per step from crops resampled straight to 112 px."""
    from scripts.evaluation import linear_probe
    cfg = full_cfg(tmp_path)
    cfg["probe"] = dict(total_epochs=2, warmup_epochs=1, batch_size=16)
    path = tmp_path / "probe112.yaml"
    path.write_text(yaml.safe_dump(cfg))
    res = linear_probe.main(["--config", str(path), "--checkpoint", "random", "--synthetic_images", "100", "--max_epochs", "1", "--augment", "crop",
                             "--output_dir_suffix", "probe112"])
    assert res["augment"] == "crop" and res["epochs"] == 1 and res["train_size"] == 60
    assert res["test_acc"] is not None and math.isfinite(res["test_loss"])
    assert (tmp_path / "outputs" / "probe" / "probe112" / "checkpoints" / "last.ckpt").exists()


def test_cli_pretrain_at_112(dev, tmp_path):
    cfg = full_cfg(tmp_path)
    cfg["pretrain"]["batch_size"] = 16
    path = tmp_path / "mae112.yaml"
    path.write_text(yaml.safe_dump(cfg))
    r = subprocess.run([sys.executable, "-m", "scripts.training.pretrain_mae", "--config", str(path), "--synthetic_images", "64", "--max_epochs", "1"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert (tmp_path / "outputs" / "pretrain" / "mae_pretrain" / "checkpoints" / "last.ckpt").exists()
