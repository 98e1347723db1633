"""An accumulated window under data parallelism on the GPU (-m gpu): two gloo ranks sharing cuda:0, each a fresh child process
(tests/accum_dp_worker.py), MICRO fp32, one window of global rows (4, 3, 1) -- rank 1 holds no row of the micro-batch that closes it and
joins the exchange with the stash alone.  Four runs, one after another: overlapped exchange in small buckets, one blocking
all-reduce, the sharded optimizer, and the single-process window.  Micro-batches that do not close the window never communicate;
overlapped and blocking agree bit for bit; every run is within 1e-5 of the single process (the tolerance of
tests/test_gpu_dp.py::test_two_rank_product_step_equals_single_process[micro]); the returned loss is the global window mean."""
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest
import torch

from tests.util import rel_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(out, world, env_extra):
    out.mkdir()
    port = _free_port()
    env = dict(os.environ, **env_extra)
    procs = [subprocess.Popen([sys.executable, str(ROOT / "tests" / "accum_dp_worker.py"), "--rank", str(r), "--world", str(world),
                               "--port", str(port), "--out", str(out)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for r in range(world)]
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for p, o in zip(procs, logs):
        assert p.returncode == 0, f"rank failed ({p.returncode}):\n{o[-3000:]}"
    return [torch.load(out / f"w{world}_r{r}.pt", weights_only=True) for r in range(world)]


def test_two_rank_window_equals_single_process_window(tmp_path):
    ov = _run(tmp_path / "overlap", 2, {"MAE_DP_OVERLAP": "1", "MAE_DP_BUCKET_MB": "0.01"})
    bl = _run(tmp_path / "blocking", 2, {"MAE_DP_OVERLAP": "0"})
    sh = _run(tmp_path / "sharded", 2, {"MAE_DP_SHARDED_OPT": "1"})
    one = _run(tmp_path / "single", 1, {})[0]
    assert ov[0]["overlap"] and not bl[0]["overlap"] and len(ov[0]["buckets"]) >= 3
    assert ov[0]["rows"].tolist() == [2, 2, 1] and ov[1]["rows"].tolist() == [2, 1, 0] and one["rows"].tolist() == [4, 3, 1]
    for run in (ov, bl, sh, [one]):
        for r in run:
            assert r["steps"].tolist() == [1, 1]                                          # one optimizer step for the window
    # overlapped (stash added bucket by bucket on the communication stream) == blocking (stash added whole), bit for bit, on both ranks
    for r in (0, 1):
        assert torch.equal(ov[r]["params"], bl[r]["params"]) and torch.equal(ov[r]["exp_avg"], bl[r]["exp_avg"])
        assert torch.equal(ov[r]["stats"], bl[r]["stats"]) and torch.equal(ov[r]["losses"], bl[r]["losses"])
    assert torch.equal(ov[0]["params"], ov[1]["params"]) and torch.equal(sh[0]["params"], sh[1]["params"])
    assert not torch.equal(one["params"], torch.zeros_like(one["params"]))
    for name, run in (("overlapped", ov), ("blocking", bl), ("sharded", sh)):
        err = rel_err(run[0]["params"], one["params"])
        print(f"{name} window vs single-process window: parameters {err:.3e}, loss {float(run[0]['losses'][-1]):.8f} vs {float(one['losses'][-1]):.8f}")
        assert err < 1e-5, name
        # the loss of the call that closes the window is the GLOBAL window mean, the same on every rank
        assert torch.equal(run[0]["losses"][-1], run[1]["losses"][-1])
        assert torch.allclose(run[0]["losses"][-1], one["losses"][-1], rtol=1e-5, atol=0)
        assert abs(float(run[0]["stats"][0]) - float(one["stats"][0])) <= 1e-4 * float(one["stats"][0])
    # the single-process window mean against the plain native loss of the 8-row batch with the same noise (no accumulation involved)
    assert torch.allclose(one["losses"][-1], one["full_loss"][0], rtol=1e-5, atol=0)
    # before the window closes a rank reports the mean of its own rows
    assert float(ov[0]["losses"][0]) != float(ov[1]["losses"][0])
