"""bench.py's command line: the --dump-outputs files (CPU), and a plain run against a --full run on a small batch (MI355X)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "kernels", "hbm_budget", "cpu_baseline")


def _import_bench(monkeypatch):
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # bench.py sets it on import: keep it out of the rest of the session
    import bench
    return bench


def test_dump_outputs_float32_and_fixed_sample(tmp_path, monkeypatch):
    bench = _import_bench(monkeypatch)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    big = torch.arange(5000, dtype=torch.float64)
    loss = torch.tensor([1.5], dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big.clone(), "loss": loss})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (1000,)
    assert np.array_equal(a, b)                 # the same positions on every call
    assert np.all(np.diff(a) > 0)               # ascending positions, none twice
    assert np.load(tmp_path / "a" / "loss.npy").tolist() == [1.5]   # small arrays are written whole


def _bench(*args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--batch", "64", "--steps", "3", "--warmup", "1", *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_is_lean_full_run_reports_the_rest_and_dumps_repeat(tmp_path):
    a = _bench("--dump-outputs", str(tmp_path / "a"))
    b = _bench("--dump-outputs", str(tmp_path / "b"))
    for line in (a, b):
        assert all(k in line for k in HEADLINE) and line["steps"] == 3 and line["ms_per_step"] > 0
        assert not any(k in line for k in FULL_ONLY)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["grads.npy", "loss.npy", "params.npy"]
    assert sum((tmp_path / "a" / n).stat().st_size for n in names) <= 64 << 20
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype == np.float32 and np.isfinite(x).all()
        assert np.array_equal(x, y), f"{n} differs between two runs with the same arguments"
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(a["final_loss"], rel=1e-6)
    full = _bench("--full", "--no-cpu-baseline")
    assert all(k in full for k in ("roofline", "kernels", "hbm_budget")) and "cpu_baseline" not in full
