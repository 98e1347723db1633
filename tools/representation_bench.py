"""Timing of the representation-evaluation kernels, printed as one JSON document.

  * feature extraction (mae_engine_extract_features) at B = 2000, bf16, pool cls and mean-over-patches, for the
    configs/mae.yaml encoder and ViT-S/8 (configs/vits8_dec192.yaml), alternated in the same process with the classifier's
    evaluation forward (mae_engine_classifier_forward), its yardstick;
  * I-JEPA ViT-S/8 (configs/ijepa_vits8.yaml) target-encoder features, patch tokens only;
  * mae_knn_topk at (Q, N, D, k) = (8000, 5000, 384, 20 / 200) and (8000, 100000, 384, 20), alternated with torch.mm +
    torch.topk (a measurement-only baseline that materialises Q x N), with the achieved 2QND / t as a share of the
    157.3 TF fp32-MFMA peak.
  * with --layers "SPEC;SPEC;..." (part `layers`): ViT-S/8 features after encoder blocks (mae_engine_extract_layer_features, one entry
    per SPEC of representation.parse_layers, e.g. "each;5") alternated with the plain last-block call, and the feature kernel alone
    (through mae_features_tap and through mae_features_pool on the same buffers) with its bytes/s.
  * part `attention`: ViT-S/8 attention maps (mae_engine_extract_attention) of the last block, of every block, and of the last block
    with rollout, alternated with the plain extract_features call; and the map kernel alone (mae_attention_colsum) with a dense and with
    a one-hot weight row on a random qkv of the engine's shape, next to the forward attention kernel (mae_attention_fwd) on the same
    qkv, with its flops/s and bytes/s.
Device events time `--steps` calls after `--warmup` calls; every number is the median of `--repeats` alternated runs.

    python tools/representation_bench.py --out profiles/r05_representation_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ssrl_vit_mae_jepa_amd.classifier import ViTClassifierTrainModule, encoder_mae  # noqa: E402
from ssrl_vit_mae_jepa_amd.jepa import IJEPA  # noqa: E402
from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.mae import _ptr, _stream  # noqa: E402
from ssrl_vit_mae_jepa_amd.representation import knn_topk, parse_layers  # noqa: E402

FP32_MFMA_PEAK_TF = 157.3


def timed(fn, steps: int, warmup: int) -> float:
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternate(cases, steps, warmup, repeats):
    runs = {}
    for _r in range(repeats):
        for key, fn in cases:
            runs.setdefault(key, []).append(timed(fn, steps, warmup))
    return {k: statistics.median(v) for k, v in runs.items()}, runs


def model_cfg(cfg_path: Path) -> dict:
    cfg = yaml.safe_load(cfg_path.read_text())
    return dict(cfg["model"], general=dict(cfg["model"]["general"], engine_precision=cfg.get("engine", {}).get("precision", "bf16")))


def bench_extraction(name: str, cfg_path: Path, B: int, steps: int, warmup: int, repeats: int) -> dict:
    mc = model_cfg(cfg_path)
    dev = torch.device("cuda", 0)
    mod = ViTClassifierTrainModule(pretrained_encoder=encoder_mae(mc).encoder.vit, model_cfg=mc, training_cfg={}).to(dev)
    mod.freeze_encoder()
    mae = mod.model.mae
    S = mc["general"]["image_size"]
    g = torch.Generator(device=dev).manual_seed(0)
    images = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=g)

    def evaluate():
        with torch.no_grad():
            mod.model.evaluate(images, None, logits=True)

    cases = [("classifier_eval_forward", evaluate),
             ("extract_cls", lambda: mae.extract_features(images, pool="cls")),
             ("extract_mean_patches", lambda: mae.extract_features(images, pool="mean")),
             ("extract_mean_patches_l2", lambda: mae.extract_features(images, pool="mean", normalize="l2"))]
    ms, runs = alternate(cases, steps, warmup, repeats)
    res = {"model": name, "config": str(cfg_path.relative_to(ROOT)), "batch": B, "precision": mae.engine.precision,
           "ms": ms, "images_per_s": {k: B / (v / 1e3) for k, v in ms.items()}, "ms_all": runs}
    del mod, mae
    torch.cuda.empty_cache()
    return res


def bench_ijepa(B: int, steps: int, warmup: int, repeats: int) -> dict:
    cfg_path = ROOT / "configs" / "ijepa_vits8.yaml"
    mc = model_cfg(cfg_path)
    dev = torch.device("cuda", 0)
    model = IJEPA(mc["general"], mc["encoder"], mc["predictor"]).to(dev)
    S = mc["general"]["image_size"]
    images = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    ms, runs = alternate([("extract_target_mean", lambda: model.extract_features(images, encoder="target")),
                          ("extract_context_mean", lambda: model.extract_features(images, encoder="context"))], steps, warmup, repeats)
    res = {"model": "ijepa_vits8", "config": str(cfg_path.relative_to(ROOT)), "batch": B, "precision": model.net.engine.precision,
           "ms": ms, "images_per_s": {k: B / (v / 1e3) for k, v in ms.items()}, "ms_all": runs}
    del model
    torch.cuda.empty_cache()
    return res


def bench_layers(specs, B: int, steps: int, warmup: int, repeats: int) -> dict:
    """ViT-S/8, mean over the patch tokens: the plain call, one layers=... call per spec, and the pooling kernels alone."""
    cfg_path = ROOT / "configs" / "vits8_dec192.yaml"
    mc = model_cfg(cfg_path)
    dev = torch.device("cuda", 0)
    mae = encoder_mae(mc).to(dev)
    depth, D, T = mae._dims["depth"], mae._dims["embed_dim"], mae.sequence_length
    S = mc["general"]["image_size"]
    images = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    cases = [("extract_mean_patches", lambda: mae.extract_features(images, pool="mean"))]
    layer_sets = {}
    for spec in specs:
        layers = parse_layers(spec, depth)
        layer_sets[f"layers_{spec}"] = list(layers)
        cases.append((f"layers_{spec}", lambda layers=layers: mae.extract_features(images, pool="mean", layers=layers)))
        if mae.encoder.vit.with_cls:
            cases.append((f"layers_{spec}_cls_mean", lambda layers=layers: mae.extract_features(images, pool="cls_mean", layers=layers)))
    # the kernels alone, on buffers of the engine's shapes: x_mid fp32, the MLP branch in the activation type
    bf = mae.engine.precision == "bf16"
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, T, D, device=dev, generator=g)
    br = torch.randn(B, T, D, device=dev, generator=g).to(torch.bfloat16 if bf else torch.float32)
    gamma, beta = torch.randn(D, device=dev, generator=g), torch.randn(D, device=dev, generator=g)
    out = torch.empty(B, 12, 2 * D, device=dev)
    dt, st = (_lib.MAE_BF16 if bf else _lib.MAE_F32), _stream(dev)

    def tap(pool, stride):
        _lib.check(_lib.lib.mae_features_tap(_ptr(x), _ptr(br), dt, _ptr(gamma), _ptr(beta), 1e-6, B, T, D, 1, pool, 0, _ptr(out), stride, st))

    def pool_kernel():
        _lib.check(_lib.lib.mae_features_pool(_ptr(x), _ptr(br), dt, _ptr(gamma), _ptr(beta), 1e-6, B, T, D, 1, T, 0, _ptr(out), st))

    cases += [("kernel_features_pool_mean_patches", pool_kernel),
              ("kernel_features_tap_mean_patches", lambda: tap(_lib.POOL_MEAN_PATCHES, 12 * D)),
              ("kernel_features_tap_cls_mean", lambda: tap(_lib.POOL_CLS_MEAN_PATCHES, 12 * 2 * D))]
    ms, runs = alternate(cases, steps, warmup, repeats)
    act = 2 if bf else 4
    kernel_bytes = {"kernel_features_pool_mean_patches": B * ((T - 1) * D * (4 + act) + D * 4),
                    "kernel_features_tap_mean_patches": B * ((T - 1) * D * (4 + act) + D * 4),
                    "kernel_features_tap_cls_mean": B * (T * D * (4 + act) + 2 * D * 4)}
    res = {"model": "vits8", "config": str(cfg_path.relative_to(ROOT)), "batch": B, "precision": mae.engine.precision, "pool": "mean",
           "layers": layer_sets, "ms": ms, "ms_over_plain": {k: v - ms["extract_mean_patches"] for k, v in ms.items() if k.startswith("layers_")},
           "kernel_bytes": kernel_bytes, "kernel_tb_per_s": {k: b / (ms[k] / 1e3) / 1e12 for k, b in kernel_bytes.items()}, "ms_all": runs}
    del mae, x, br, out
    torch.cuda.empty_cache()
    return res


def bench_attention(B: int, steps: int, warmup: int, repeats: int) -> dict:
    """ViT-S/8: extract_attention next to extract_features, and the colsum kernel next to the forward attention kernel."""
    cfg_path = ROOT / "configs" / "vits8_dec192.yaml"
    mc = model_cfg(cfg_path)
    dev = torch.device("cuda", 0)
    mae = encoder_mae(mc).to(dev)
    depth, D, H, T = mae._dims["depth"], mae._dims["embed_dim"], mae._dims["num_heads"], mae.sequence_length
    hd, S = D // H, mc["general"]["image_size"]
    images = torch.randint(0, 256, (B, 3, S, S), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    cases = [("extract_cls", lambda: mae.extract_features(images, pool="cls")),
             ("attention_last", lambda: mae.extract_attention(images)),
             ("attention_each", lambda: mae.extract_attention(images, layers=range(depth))),
             ("attention_last_rollout", lambda: mae.extract_attention(images, rollout=True)),
             ("attention_last_mean_query", lambda: mae.extract_attention(images, query="mean"))]
    bf = mae.engine.precision == "bf16"
    g = torch.Generator(device=dev).manual_seed(3)
    qkv = torch.randn(B, T, 3 * D, device=dev, generator=g).to(torch.bfloat16 if bf else torch.float32)
    dense = torch.full((B, T), 1.0 / T, device=dev)
    onehot = torch.zeros(B, T, device=dev)
    onehot[:, 0] = 1.0
    per_head, mixed = torch.empty(B, H, T, device=dev), torch.empty(B, T, device=dev)
    att, lse = torch.empty(B, T, D, device=dev, dtype=qkv.dtype), torch.empty(B, H, T, device=dev)
    dt, st = (_lib.MAE_BF16 if bf else _lib.MAE_F32), _stream(dev)

    def colsum(w):
        _lib.check(_lib.lib.mae_attention_colsum(_ptr(qkv), dt, B, T, H, hd, _ptr(w), _ptr(per_head), H * T, _ptr(mixed), st))

    def attention_fwd():
        _lib.check(_lib.lib.mae_attention_fwd(_ptr(qkv), B, T, H, hd, dt, _ptr(att), _ptr(lse), st))

    cases += [("kernel_attention_fwd", attention_fwd), ("kernel_colsum_dense", lambda: colsum(dense)), ("kernel_colsum_onehot", lambda: colsum(onehot))]
    ms, runs = alternate(cases, steps, warmup, repeats)
    act = 2 if bf else 4
    out_bytes = B * T * 4 * (2 + H)
    work = {"kernel_attention_fwd": dict(flops=4.0 * B * H * T * T * hd, bytes=B * T * 4 * D * act + B * H * T * 4),
            "kernel_colsum_dense": dict(flops=B * H * T * T * (2.0 * hd + 6), bytes=B * 2 * T * D * act + out_bytes),
            "kernel_colsum_onehot": dict(flops=B * H * T * (2.0 * hd + 6), bytes=B * (T + 1) * D * act + out_bytes)}
    res = {"model": "vits8", "config": str(cfg_path.relative_to(ROOT)), "batch": B, "precision": mae.engine.precision, "shape": [B, T, H, hd],
           "ms": ms, "ms_over_extract_cls": {k: v - ms["extract_cls"] for k, v in ms.items() if k.startswith("attention_")},
           "kernel_over_attention_fwd": {k: ms[k] / ms["kernel_attention_fwd"] for k in work},
           "kernel_work": work, "kernel_tflops": {k: w["flops"] / (ms[k] / 1e3) / 1e12 for k, w in work.items()},
           "kernel_tb_per_s": {k: w["bytes"] / (ms[k] / 1e3) / 1e12 for k, w in work.items()}, "ms_all": runs}
    del mae, qkv, att
    torch.cuda.empty_cache()
    return res


def bench_topk(Q: int, N: int, D: int, k: int, steps: int, warmup: int, repeats: int) -> dict:
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(2)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device=dev, generator=g), dim=1)
    b = torch.nn.functional.normalize(torch.randn(N, D, device=dev, generator=g), dim=1)

    def baseline():
        torch.topk(torch.mm(q, b.T), k, dim=1)

    ms, runs = alternate([("knn_topk", lambda: knn_topk(q, b, k)), ("torch_mm_topk", baseline)], steps, warmup, repeats)
    flop = 2.0 * Q * N * D
    res = {"Q": Q, "N": N, "D": D, "k": k, "ms": ms, "ms_all": runs,
           "tflops": {key: flop / (v / 1e3) / 1e12 for key, v in ms.items()}}
    res["share_of_fp32_mfma_peak"] = {key: t / FP32_MFMA_PEAK_TF for key, t in res["tflops"].items()}
    del q, b
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batch", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parts", default="extract,ijepa,topk")
    ap.add_argument("--layers", default=None, help='part `layers`: ";"-separated layer specs, e.g. "each;5"')
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.backends.cuda.matmul.allow_tf32 = False
    parts = set(args.parts.split(","))
    out = {"tool": "tools/representation_bench.py", "argv": sys.argv[1:] if argv is None else list(argv),
           "device": torch.cuda.get_device_name(0), "extraction": [], "topk": []}
    if "extract" in parts:
        for name, path in (("yaml", ROOT / "configs" / "mae.yaml"), ("vits8", ROOT / "configs" / "vits8_dec192.yaml")):
            out["extraction"].append(bench_extraction(name, path, args.batch, args.steps, args.warmup, args.repeats))
    if "ijepa" in parts:
        out["extraction"].append(bench_ijepa(args.batch, args.steps, args.warmup, args.repeats))
    if "layers" in parts or args.layers:
        if not args.layers:
            ap.error("part `layers` needs --layers")
        out["layers"] = bench_layers([t for t in args.layers.split(";") if t], args.batch, args.steps, args.warmup, args.repeats)
    if "attention" in parts:
        out["attention"] = bench_attention(args.batch, args.steps, args.warmup, args.repeats)
    if "topk" in parts:
        for shape in ((8000, 5000, 384, 20), (8000, 5000, 384, 200), (8000, 100_000, 384, 20)):
            out["topk"].append(bench_topk(*shape, args.steps, args.warmup, args.repeats))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
