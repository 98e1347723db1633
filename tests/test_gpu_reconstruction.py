"""MAE reconstruction on the GPU (-m gpu): the compose kernel (mae_reconstruct_compose) against the CPU reference of
tests/recon_ref.py, its argument checks, MaskedAutoencoder.reconstruct (mae_engine_reconstruct) against the two forwards it is
made of and against the oracle, and the CLI.

Tolerances: composed images bit-exact (fp32 values are copies, uint8 values the torch fp32 display expression); every per-image
sum within gamma_n = n u / (1 - n u), u = 2^-24, n = replaced pixels per image + 2, of the fp64 sum of the same fp32 terms
(worst case of an fp32 sum of non-negative terms in any order, plus the subtract and the square); n <= 3074 here -> 1.9e-4."""
import ctypes as C
import functools
import json
import math

import pytest
import torch

from oracle import mae_oracle as O
from tests import recon_ref as R
from tests.test_gpu_engine import MICRO, build
from tests.util import rel_err

pytestmark = pytest.mark.gpu

SHAPES = [(3, 32, 8),    # the vector path
          (3, 30, 6),    # the scalar path
          (1, 30, 6),    # one channel
          (3, 32, 16)]   # N = 4
B = 3
MASKS = ("one", "half", "all", "junk")


def _indices(kind: str, N: int, g: torch.Generator) -> torch.Tensor:
    m = {"one": 1, "half": N // 2, "all": N, "junk": N // 2}[kind]
    idx = torch.stack([torch.randperm(N, generator=g)[:m] + 1 for _ in range(B)])
    if kind == "junk":  # a class-token entry (0) and an id past the grid (N + 1) among the valid ones, at other columns in every row
        rows = []
        for b in range(B):
            r = idx[b].tolist()
            r.insert(b % (m + 1), 0)
            r.insert((b + 2) % (m + 2), N + 1)
            rows.append(r)
        idx = torch.tensor(rows)
    return idx


@functools.lru_cache(maxsize=None)
def case(C_, S, p, in_u8: bool, kind: str):
    """One seeded problem and its reference, computed once and shared by the tests (never modified)."""
    g = torch.Generator().manual_seed(1000 + 7 * S + p + 3 * C_ + MASKS.index(kind))
    N = (S // p) ** 2
    images = torch.randint(0, 256, (B, C_, S, S), generator=g, dtype=torch.uint8) if in_u8 else torch.rand(B, C_, S, S, generator=g) * 2 - 1
    idx = _indices(kind, N, g)
    pred = torch.randn(B, idx.shape[1], p * p * C_, generator=g) * 0.7
    recon, masked = R.compose_ref(images, pred, idx, p, fill=0.5)
    sq, ab = R.sums_ref(images, recon)
    n_valid = int(((idx[0] >= 1) & (idx[0] <= N)).sum())
    return dict(images=images, idx=idx, pred=pred, recon=recon, masked=masked, sq=sq, ab=ab, n=n_valid * p * p * C_ + 2)


def check_sums(got_sq, got_ab, c):
    bound = R.gamma(c["n"])
    assert c["n"] <= 3074 and bound < 1.9e-4
    for got, ref in ((got_sq, c["sq"]), (got_ab, c["ab"])):
        err = (got.double().cpu() - ref).abs() / ref
        print("sum rel err", err.tolist(), "bound", bound)
        assert (err <= bound).all(), (err.tolist(), bound)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("out", ["float", "uint8"])
@pytest.mark.parametrize("in_u8", [False, True], ids=["f32in", "u8in"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_S%d_p%d" % s)
def test_compose_matches_reference(dev, shape, in_u8, out, kind):
    from ssrl_vit_mae_jepa_amd.mae import unpatchify_compose
    c = case(*shape, in_u8, kind)
    r = unpatchify_compose(c["images"].to(dev), c["pred"].to(dev), c["idx"].to(dev), shape[2], fill=0.5, out=out)
    want_r, want_m = (c["recon"], c["masked"]) if out == "float" else (R.display_u8(c["recon"]), R.display_u8(c["masked"]))
    assert r.reconstructed.dtype == want_r.dtype and torch.equal(r.reconstructed.cpu(), want_r)
    assert r.masked.dtype == want_m.dtype and torch.equal(r.masked.cpu(), want_m)
    assert r.sum_sq.shape == (B,) and r.sum_abs.shape == (B,)
    check_sums(r.sum_sq, r.sum_abs, c)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_S%d_p%d" % s)
def test_null_outputs(dev, shape):
    from ssrl_vit_mae_jepa_amd.mae import unpatchify_compose
    c = case(*shape, True, "half")
    args = (c["images"].to(dev), c["pred"].to(dev), c["idx"].to(dev), shape[2])
    full = unpatchify_compose(*args)
    only_r = unpatchify_compose(*args, masked=False, stats=False)
    only_m = unpatchify_compose(*args, reconstructed=False)
    only_s = unpatchify_compose(*args, reconstructed=False, masked=False)
    assert only_r.masked is None and only_r.sum_sq is None and torch.equal(only_r.reconstructed, full.reconstructed)
    assert only_m.reconstructed is None and torch.equal(only_m.masked, full.masked) and torch.equal(only_m.sum_sq, full.sum_sq)
    assert only_s.reconstructed is None and only_s.masked is None
    assert torch.equal(only_s.sum_sq, full.sum_sq) and torch.equal(only_s.sum_abs, full.sum_abs)
    assert torch.equal(full.reconstructed.cpu(), c["recon"])


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d_S%d_p%d" % s)
def test_sums_deterministic_and_independent_of_the_batch(dev, shape):
    from ssrl_vit_mae_jepa_amd.mae import unpatchify_compose
    c = case(*shape, False, "half")
    img, pred, idx = c["images"].to(dev), c["pred"].to(dev), c["idx"].to(dev)
    a = unpatchify_compose(img, pred, idx, shape[2])
    b = unpatchify_compose(img, pred, idx, shape[2])
    assert torch.equal(a.sum_sq, b.sum_sq) and torch.equal(a.sum_abs, b.sum_abs)
    # image 1 as the fourth of five: the order of its sum depends on the image alone
    g = torch.Generator().manual_seed(9)
    N = (shape[1] // shape[2]) ** 2
    img5 = (torch.rand(5, *img.shape[1:], generator=g) * 2 - 1).to(dev)
    pred5 = torch.randn(5, *pred.shape[1:], generator=g).to(dev)
    idx5 = torch.stack([torch.randperm(N, generator=g)[:idx.shape[1]] + 1 for _ in range(5)]).to(dev)
    img5[3], pred5[3], idx5[3] = img[1], pred[1], idx[1]
    five = unpatchify_compose(img5, pred5, idx5, shape[2])
    assert torch.equal(five.sum_sq[3], a.sum_sq[1]) and torch.equal(five.sum_abs[3], a.sum_abs[1])
    assert torch.equal(five.reconstructed[3], a.reconstructed[1])


def test_python_layer_checks(dev):
    from ssrl_vit_mae_jepa_amd.mae import unpatchify_compose
    c = case(3, 32, 8, False, "half")
    img, pred, idx = c["images"].to(dev), c["pred"].to(dev), c["idx"].to(dev)
    dup = idx.clone()
    dup[1, 0] = dup[1, 1]
    with pytest.raises(ValueError, match="distinct"):
        unpatchify_compose(img, pred, dup, 8)
    # repeated IGNORED entries (two class tokens, two ids past the grid) are not duplicates: they and their pred rows leave no trace
    junk = torch.cat([idx, torch.tensor([[0, 0, 17, 17]] * B, device=dev)], dim=1)
    junk_pred = torch.cat([pred, torch.full((B, 4, pred.shape[2]), 99.0, device=dev)], dim=1)
    r = unpatchify_compose(img, junk_pred, junk, 8)
    assert torch.equal(r.reconstructed.cpu(), c["recon"]) and torch.equal(r.masked.cpu(), c["masked"])
    with pytest.raises(ValueError, match="distinct"):
        unpatchify_compose(img, junk_pred, torch.cat([idx, idx[:, :1], torch.tensor([[0, 17, 17]] * B, device=dev)], dim=1), 8)
    assert torch.equal(unpatchify_compose(img, pred, idx, 8, check_distinct=False).reconstructed.cpu(), c["recon"])
    with pytest.raises(ValueError):
        unpatchify_compose(img, pred[:, :-1], idx, 8)
    with pytest.raises(ValueError):
        unpatchify_compose(img, pred, idx, 8, out="int8")
    with pytest.raises(ValueError):
        unpatchify_compose(img, pred, idx, 7)
    with pytest.raises(RuntimeError):
        unpatchify_compose(img.cpu(), pred, idx, 8)


def test_argument_errors_before_any_launch(dev):
    """Values the host rejects: nothing is launched, the message names the argument."""
    from ssrl_vit_mae_jepa_amd import _lib
    lib = _lib.lib
    S, p, m = 32, 8, 4
    img = torch.zeros(1, 3, S, S, device=dev)
    pred = torch.zeros(1, m, p * p * 3, device=dev)
    idx = torch.arange(1, m + 1, device=dev).view(1, m)
    out = torch.full_like(img, 7.0)
    stats = torch.full((1, 2), 7.0, device=dev)
    scratch = torch.empty(lib.mae_reconstruct_scratch_bytes(1, 3, S, p), dtype=torch.uint8, device=dev)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def call(S_=S, p_=p, m_=m, recon=out):
        return lib.mae_reconstruct_compose(ptr(img), _lib.MAE_F32, ptr(pred), ptr(idx), 1, 3, S_, p_, m_, 0.5, _lib.MAE_F32, ptr(recon), None,
                                           ptr(stats), ptr(scratch), scratch.numel(), None)

    big = torch.full((2 * img.numel(),), 7.0, device=dev)   # a buffer that holds pred in its middle: an output overlapping it in part
    pred_in = big[img.numel() - 64:img.numel() - 64 + pred.numel()].view_as(pred)
    assert lib.mae_reconstruct_compose(ptr(img), _lib.MAE_F32, ptr(pred_in), ptr(idx), 1, 3, S, p, m, 0.5, _lib.MAE_F32, ptr(big), None,
                                       ptr(stats), ptr(scratch), scratch.numel(), None) != 0
    assert b"overlap pred" in lib.mae_last_error()
    assert lib.mae_reconstruct_compose(ptr(img), _lib.MAE_F32, ptr(pred), ptr(idx), 1, 3, S, p, m, 0.5, _lib.MAE_F32, ptr(big), ptr(big[16:]),
                                       ptr(stats), ptr(scratch), scratch.numel(), None) != 0
    assert b"different buffers" in lib.mae_last_error()
    torch.cuda.synchronize()
    assert bool((big == 7.0).all())
    for kwargs, text in ((dict(S_=30), b"not divisible"), (dict(m_=0), b"num_mask"), (dict(recon=img), b"out != images")):
        assert call(**kwargs) != 0
        assert text in lib.mae_last_error(), lib.mae_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((stats == 7.0).all()) and bool((img == 0).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and stats.tolist() == [[0.0, 0.0]]


# ------------------------------------------------------------------------------------------------------------------
# engine level
# ------------------------------------------------------------------------------------------------------------------
ENGINE_CASES = [(MICRO, 2, 0.75), (MICRO, 5, 0.5), (O.YAML_TINY, 2, 0.75), (O.YAML_TINY, 5, 0.5)]
IDS = ["micro_B2_r75", "micro_B5_r50", "tiny_B2_r75", "tiny_B5_r50"]


@functools.lru_cache(maxsize=None)
def oracle_case(i: int):
    cfg, Bn, r = ENGINE_CASES[i]
    params = O.init_params(cfg, 73)
    O.randomize_params(params)
    images = O.synthetic_images(Bn, cfg)
    noise = O.make_noise(Bn, cfg.sequence_length, torch.Generator().manual_seed(74))
    keep, mask = O.mask_from_noise(noise, cfg.num_keep(r))
    with torch.no_grad():
        x_pred = O.forward_decoder(params, cfg, O.forward_encoder(params, cfg, images, keep), keep, mask)
    return dict(images=images, noise=noise, keep=keep, mask=mask, x_pred=x_pred)


@pytest.mark.parametrize("i", range(len(ENGINE_CASES)), ids=IDS)
def test_reconstruct_fp32_is_the_two_forwards_plus_compose(dev, i):
    cfg, Bn, r = ENGINE_CASES[i]
    oc = oracle_case(i)
    model, _ = build(cfg, "fp32", dev, r)
    images, keep, mask = oc["images"].to(dev), oc["keep"].to(dev), oc["mask"].to(dev)
    with torch.no_grad():
        want = model.forward_decoder(model.forward_encoder(images, keep), keep, mask)
    res = model.reconstruct(images, keep, mask)
    assert torch.equal(res.x_pred, want)  # the same kernels
    assert torch.equal(res.idx_keep, keep) and torch.equal(res.idx_mask, mask)
    recon, masked = R.compose_ref(oc["images"], res.x_pred, oc["mask"], cfg.patch_size)
    assert torch.equal(res.reconstructed.cpu(), recon) and torch.equal(res.masked.cpu(), masked)
    assert rel_err(res.x_pred, oc["x_pred"]) < 1e-4
    # the mask drawn from noise inside reconstruct is the oracle's
    again = model.reconstruct(images, noise=oc["noise"], mask_ratio=r, out="uint8")
    assert torch.equal(again.idx_mask.cpu(), oc["mask"]) and torch.equal(again.x_pred, res.x_pred)
    assert torch.equal(again.reconstructed.cpu(), R.display_u8(recon)) and torch.equal(again.sum_sq, res.sum_sq)
    with pytest.raises(ValueError, match="distinct"):
        bad = mask.clone()
        bad[0, 0] = bad[0, 1]
        model.reconstruct(images, keep, bad)
    with pytest.raises(ValueError, match="partition"):
        model.reconstruct(images, keep, mask[:, :-1])


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_engine_reconstruct_with_x_pred_in_the_workspace(dev, precision):
    """mae_engine_reconstruct with x_pred = NULL (the prediction then lives in the workspace): the same images and sums."""
    from ssrl_vit_mae_jepa_amd import _lib
    from ssrl_vit_mae_jepa_amd._lib import check, lib
    cfg, Bn, r = ENGINE_CASES[3]
    oc = oracle_case(3)
    model, _ = build(cfg, precision, dev, r)
    images, keep, mask = oc["images"].to(dev), oc["keep"].to(dev), oc["mask"].to(dev)
    want = model.reconstruct(images, keep, mask)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    k, m = keep.shape[1], mask.shape[1]
    ws = model._ws(Bn, k)
    wc = model._weights()
    recon, masked = torch.empty_like(images), torch.empty_like(images)
    stats = torch.empty(Bn, 2, device=dev)
    scratch = torch.empty(lib.mae_reconstruct_scratch_bytes(Bn, cfg.in_chans, cfg.image_size, cfg.patch_size), dtype=torch.uint8, device=dev)
    check(lib.mae_engine_reconstruct(model.engine.handle, ptr(model.flat_params), ptr(wc), ptr(images), _lib.MAE_F32, ptr(keep), ptr(mask), Bn, k, m,
                                     0.5, _lib.MAE_F32, ptr(ws), ws.numel(), None, ptr(recon), ptr(masked), ptr(stats), ptr(scratch),
                                     scratch.numel(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    assert torch.equal(recon, want.reconstructed) and torch.equal(masked, want.masked)
    assert torch.equal(stats[:, 0], want.sum_sq) and torch.equal(stats[:, 1], want.sum_abs)


@pytest.mark.parametrize("i", range(len(ENGINE_CASES)), ids=IDS)
def test_reconstruct_bf16_close_to_oracle(dev, i):
    cfg, Bn, r = ENGINE_CASES[i]
    oc = oracle_case(i)
    model, _ = build(cfg, "bf16", dev, r)
    res = model.reconstruct(oc["images"].to(dev), oc["keep"].to(dev), oc["mask"].to(dev))
    assert rel_err(res.x_pred, oc["x_pred"]) < 2e-2
    recon, masked = R.compose_ref(oc["images"], res.x_pred, oc["mask"], cfg.patch_size)
    assert torch.equal(res.reconstructed.cpu(), recon) and torch.equal(res.masked.cpu(), masked)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("i", range(len(ENGINE_CASES)), ids=IDS)
def test_sum_sq_is_the_validation_loss(dev, i, precision):
    """sum_sq.sum() / (B m P) against the loss of loss_and_grads on the same noise: |diff| <= gamma_n |loss| + 1e-6."""
    cfg, Bn, r = ENGINE_CASES[i]
    oc = oracle_case(i)
    model, _ = build(cfg, precision, dev, r)
    images, noise = oc["images"].to(dev), oc["noise"].to(dev)
    loss = float(model.loss_and_grads(images, noise).item())
    res = model.reconstruct(images, noise=noise)
    m, P = res.idx_mask.shape[1], cfg.patch_size ** 2 * cfg.in_chans
    got = float(res.sum_sq.double().sum().item()) / (Bn * m * P)
    bound = R.gamma(m * P + 2) * abs(loss) + 1e-6
    print("masked mse", got, "loss", loss, "diff", abs(got - loss), "bound", bound)
    assert abs(got - loss) <= bound
    from ssrl_vit_mae_jepa_amd.reconstruction import reconstruction_stats
    st = reconstruction_stats(res.sum_sq, res.sum_abs, cfg.in_chans * cfg.image_size ** 2, m * P)
    assert math.isclose(st["masked_mse"], got, rel_tol=1e-12) and st["mse"] < st["masked_mse"]


@pytest.mark.parametrize("i", range(len(ENGINE_CASES)), ids=IDS)
def test_uint8_images_equal_host_normalised_images(dev, i):
    cfg, Bn, r = ENGINE_CASES[i]
    oc = oracle_case(i)
    model, _ = build(cfg, "fp32", dev, r)
    g = torch.Generator().manual_seed(31 + i)
    u8 = torch.randint(0, 256, (Bn, cfg.in_chans, cfg.image_size, cfg.image_size), generator=g, dtype=torch.uint8)
    keep, mask = oc["keep"].to(dev), oc["mask"].to(dev)
    for out in ("float", "uint8"):
        a = model.reconstruct(u8.to(dev), keep, mask, out=out)
        b = model.reconstruct(R.normalize_u8(u8).to(dev), keep, mask, out=out)
        for x, y in zip((a.x_pred, a.reconstructed, a.masked, a.sum_sq, a.sum_abs), (b.x_pred, b.reconstructed, b.masked, b.sum_sq, b.sum_abs)):
            assert torch.equal(x, y)


def test_reconstruct_between_forward_and_backward_makes_backward_raise(dev):
    model, _ = build(MICRO, "fp32", dev)
    oc = oracle_case(0)
    images, noise = oc["images"].to(dev), oc["noise"].to(dev)
    preds, targets = model(images, noise=noise)
    loss = torch.nn.functional.mse_loss(preds, targets)
    model.reconstruct(images, noise=noise)
    with pytest.raises(RuntimeError, match="overwrote"):
        loss.backward()


# ------------------------------------------------------------------------------------------------------------------
# evaluation helpers and the CLI
# ------------------------------------------------------------------------------------------------------------------
def test_evaluate_reconstruction_accumulates_over_batches(dev):
    from ssrl_vit_mae_jepa_amd.reconstruction import evaluate_reconstruction, reconstruction_stats
    cfg = MICRO
    model, _ = build(cfg, "fp32", dev)
    g = torch.Generator().manual_seed(8)
    u8 = torch.randint(0, 256, (7, 3, 32, 32), generator=g, dtype=torch.uint8).to(dev)
    batches = [u8[:4], (u8[4:], torch.zeros(3))]
    st = evaluate_reconstruction(model, lambda: iter(batches), mask_ratio=0.5, mask_seed=5)
    gen = torch.Generator().manual_seed(5)
    sq, ab = [], []
    for x in (u8[:4], u8[4:]):
        r = model.reconstruct(x, noise=torch.rand(x.shape[0], cfg.sequence_length, generator=gen), mask_ratio=0.5)
        sq.append(r.sum_sq); ab.append(r.sum_abs)
        assert r.idx_mask.shape[1] == cfg.sequence_length - model.num_keep(0.5)
    want = reconstruction_stats(torch.cat(sq), torch.cat(ab), 3 * 32 * 32, r.idx_mask.shape[1] * 192)
    assert st == want and st["images"] == 7


def test_cli_random_model_and_checkpoint_round_trip(dev, tmp_path, monkeypatch):
    import yaml
    from pathlib import Path
    from scripts.evaluation import visualize_reconstruction as V
    from scripts.training import pretrain_mae
    root = Path(__file__).resolve().parents[1]
    res = V.main(["--config", str(root / "configs" / "vits8_dec192.yaml"), "--model_path", "random", "--synthetic_images", "16", "--num_samples", "4",
                  "--output_dir", str(tmp_path / "viz")])
    png, js = tmp_path / "viz" / "reconstruction_validation.png", tmp_path / "viz" / "reconstruction_stats.json"
    assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n" and png.stat().st_size > 1000
    saved = json.loads(js.read_text())
    assert saved == json.loads(json.dumps(res)) and saved["layout"] == "random" and saved["sample"]["images"] == 4
    for k in ("mse", "l1", "psnr", "masked_mse"):
        assert math.isfinite(saved["sample"][k]), k
    assert "val" not in saved

    # a checkpoint written by this repository's pretraining loads strictly, in both of its file formats
    cfg = yaml.safe_load(open(root / "configs" / "mae.yaml"))
    cfg["pretrain"].update(batch_size=32, total_epochs=1, warmup_epochs=1)
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    cfg_path = tmp_path / "mae.yaml"
    yaml.safe_dump(cfg, open(cfg_path, "w"))
    monkeypatch.chdir(tmp_path)
    pretrain_mae.main(["--config", str(cfg_path), "--output_dir_suffix", "t", "--synthetic_images", "64", "--max_epochs", "1"])
    out = tmp_path / "outputs" / "pretrain" / "t"
    for ck, layout in ((out / "checkpoints" / "last.ckpt", "state_dict"), (out / "vit-mae.pt", "raw")):
        res = V.main(["--config", str(cfg_path), "--model_path", str(ck), "--synthetic_images", "40", "--num_samples", "3", "--eval_split", "val",
                      "--output_dir", str(tmp_path / layout), "--output_path_suffix", "r.png"])
        assert res["layout"] == layout and (tmp_path / layout / "r.png").exists()
        assert res["sample"]["images"] == 3 and res["val"]["images"] > 0
        assert all(math.isfinite(res[s][k]) for s in ("sample", "val") for k in ("mse", "l1", "psnr", "masked_mse"))
