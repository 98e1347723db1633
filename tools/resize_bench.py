"""Cost of the on-device resize (`mae_resize_crop_flip`, k_resize.hip), printed as one JSON document.

Device events, warm-up first, the cases alternating inside one run, every figure the median of `--repeats` timed windows:
  * (512, 3, 96 -> 224) uint8 -> uint8 and uint8 -> fp32, whole image: one ViT-B/16 batch of configs/vitb16_dec512.yaml;
  * (256, 3, 96 -> 224) uint8 -> fp32: one ViT-L/14 batch of configs/ijepa_vitl14.yaml (its engine reads no bytes);
  * (2000, 3, 96 -> 96) uint8 -> uint8 with seeded RandomResizedCrop boxes + flips, beside `mae_augment_crop_flip_u8` on the same
    inputs and boxes (the kernel the 96 px path keeps);
each with the bytes/s it achieves on its algorithmic bytes (every input byte read once, every output byte written once), beside the
copy and add rates that torch's own streaming kernels reach in the same run (the method of tools/hbm_stream_reference.py, 1 GiB).
`--step_ms`: a ViT-B/16 step measured in the same session (`bench.py --config configs/vitb16_dec512.yaml --batch 512`,
ms_per_step); the document then carries the resize's share of it.

    python tools/resize_bench.py --step_ms 46.0 --out profiles/r22_resize_bench.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from ssrl_vit_mae_jepa_amd import _lib  # noqa: E402
from ssrl_vit_mae_jepa_amd.data import draw_augment_params  # noqa: E402
from ssrl_vit_mae_jepa_amd.mae import _stream  # noqa: E402


def timed(fn, steps: int) -> float:
    """Milliseconds per call over `steps` calls between two device events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / steps


def alternate(cases: dict, steps: int, warmup: int, repeats: int) -> dict:
    for fn in cases.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in cases}
    for _ in range(repeats):
        for k, fn in cases.items():
            runs[k].append(timed(fn, steps))
    return {k: {"ms": statistics.median(v), "ms_all": v} for k, v in runs.items()}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200, help="kernel calls per timed window")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step_ms", type=float, default=None, help="ms per ViT-B/16 step (batch 512) measured in the same session by bench.py")
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: needs the MI355X (no CPU path)")
    dev = torch.device("cuda", 0)
    s = _stream(dev)
    lib, U8, F32 = _lib.lib, _lib.MAE_U8, _lib.MAE_F32
    g = torch.Generator(device=dev).manual_seed(73)

    def images(B):
        return torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, device=dev, generator=g)

    cases, algo_bytes, keep = {}, {}, []

    def resize_case(name, x, params, So, out_dt):
        B, C, Si, _ = x.shape
        out = torch.empty((B, C, So, So), dtype=torch.uint8 if out_dt == U8 else torch.float32, device=dev)
        keep.extend((x, params, out))
        p = 0 if params is None else params.data_ptr()
        cases[name] = lambda: _lib.check(lib.mae_resize_crop_flip(x.data_ptr(), U8, B, C, Si, p, So, out_dt, out.data_ptr(), s))
        algo_bytes[name] = x.numel() + out.numel() * out.element_size()

    x512, x256, x2000 = images(512), images(256), images(2000)
    resize_case("resize_512x3_96to224_u8_u8", x512, None, 224, U8)
    resize_case("resize_512x3_96to224_u8_f32", x512, None, 224, F32)
    resize_case("resize_256x3_96to224_u8_f32", x256, None, 224, F32)
    draw = draw_augment_params(2000, 96, torch.Generator(device=dev).manual_seed(80))
    boxes = torch.stack([t.to(torch.int64) for t in draw], dim=1).to(torch.int32).contiguous()
    resize_case("resize_2000x3_96to96_u8_u8_boxes", x2000, boxes, 96, U8)
    old_out = torch.empty_like(x2000)
    cases["augment_crop_flip_u8_2000x3_96"] = lambda: _lib.check(lib.mae_augment_crop_flip_u8(x2000.data_ptr(), boxes.data_ptr(), 2000, 3, 96,
                                                                                              old_out.data_ptr(), s))
    algo_bytes["augment_crop_flip_u8_2000x3_96"] = 2 * x2000.numel()

    # the yardstick: torch's own streaming kernels on 1 GiB, as tools/hbm_stream_reference.py times them, inside the same alternation
    n = 1024 * 1024 * 1024 // 4
    a, b = torch.rand(n, device=dev), torch.empty(n, device=dev)
    cases["torch_copy_1GiB"] = lambda: b.copy_(a)
    cases["torch_add_1GiB"] = lambda: torch.add(a, 1.0, out=b)
    algo_bytes["torch_copy_1GiB"] = algo_bytes["torch_add_1GiB"] = 8 * n

    res = alternate(cases, args.steps, args.warmup, args.repeats)
    for k, v in res.items():
        v["algorithmic_bytes"] = algo_bytes[k]
        v["tb_per_s"] = algo_bytes[k] / (v["ms"] * 1e-3) / 1e12
    copy = res["torch_copy_1GiB"]["tb_per_s"]
    for k, v in res.items():
        v["frac_of_torch_copy"] = v["tb_per_s"] / copy
    # the two kernels on the same inputs and boxes: different roundings of the same bilinear sum, never more than one grey level apart
    torch.cuda.synchronize()
    new_out = keep[-1]
    diff = (new_out.to(torch.int16) - old_out.to(torch.int16)).abs()
    out = {"device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "measured_with": "two HIP events around `steps` back-to-back launches; median of `repeats` windows, cases alternating", "cases": res,
           "same_size_vs_old_kernel": {"new_ms": res["resize_2000x3_96to96_u8_u8_boxes"]["ms"], "old_ms": res["augment_crop_flip_u8_2000x3_96"]["ms"],
                                       "new_over_old": res["resize_2000x3_96to96_u8_u8_boxes"]["ms"] / res["augment_crop_flip_u8_2000x3_96"]["ms"],
                                       "max_abs_byte_difference": int(diff.max()), "bytes_that_differ": int((diff > 0).sum()), "bytes": diff.numel()}}
    if args.step_ms is not None:
        ms = res["resize_512x3_96to224_u8_u8"]["ms"]
        out["vitb16_step"] = {"step_ms": args.step_ms, "source": "bench.py --config configs/vitb16_dec512.yaml --batch 512, ms_per_step, same session",
                              "resize_ms": ms, "resize_share_of_step": ms / args.step_ms, "budget": 0.01}
    text = json.dumps(out, indent=1)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    print(text)
    return out


if __name__ == "__main__":
    main()
