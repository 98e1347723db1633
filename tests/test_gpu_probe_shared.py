"""What the three probes share, on the MI355X: the scratch pool only grows, so a call on fewer rows reuses the buffers a larger call
left behind and must still give the bits a fresh probe gives; and both tools turn a ``--resume`` state the probe refuses into a
SystemExit that names the flag."""
from pathlib import Path

import pytest
import torch
import yaml

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
D, C, T = 8, 3, 3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def make(kind, dev, seed):
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe, ProbeSweep
    if kind == "linear":
        return LinearProbe(D, C, seed=seed, device=dev)
    if kind == "sweep":
        return ProbeSweep(D, C, [dict(base_learning_rate=0.1, weight_decay=0.0), dict(base_learning_rate=0.2, weight_decay=0.001)], seed=seed, device=dev)
    return AttentiveProbe(D, C, 2, seed=seed, device=dev)


def same(got, want):
    return all(torch.equal(a, b) for a, b in zip(got, want)) and len(got) == len(want) == 3


@pytest.mark.parametrize("kind", ["linear", "sweep", "attentive"])
def test_a_grown_scratch_pool_does_not_change_a_smaller_call(dev, kind):
    g = torch.Generator().manual_seed(11)
    shape = (33, T, D) if kind == "attentive" else (33, D)
    x = (torch.randn(*shape, generator=g) * 2 + 1).to(dev)
    labels = torch.randint(0, C, (33,), generator=g).to(dev)
    probe = make(kind, dev, seed=5)
    probe.step(x, labels, 0.1)                                   # running statistics and weights away from their initial values
    fresh = make(kind, dev, seed=6)
    fresh.load_state_dict(probe.state_dict())
    probe.evaluate(x, labels)                                    # the pool now holds buffers sized for 33 rows
    want = fresh.evaluate(x[:5].clone(), labels[:5].clone())     # buffers sized for 5 rows
    assert same(probe.evaluate(x[:5], labels[:5]), want)
    if kind == "sweep":                                          # labels at an address that is no multiple of 16: the sweep copies them
        assert labels[1:6].data_ptr() % 16 != 0
        assert same(probe.evaluate(x[1:6], labels[1:6]), fresh.evaluate(x[1:6].clone(), labels[1:6].clone()))


def test_linear_probe_resume_refusal_names_the_flag(dev, tmp_path):
    from scripts.evaluation import linear_probe
    from ssrl_vit_mae_jepa_amd.probe import LinearProbe
    cfg = yaml.safe_load((ROOT / "configs" / "vits8_dec192_linprobe.yaml").read_text())
    cfg["logging"]["output_dir_base"] = str(tmp_path / "outputs")
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    state = LinearProbe(384, 10).state_dict()
    state["mu"] = state["mu"][:-4]
    torch.save(state, tmp_path / "bad.pt")
    with pytest.raises(SystemExit) as e:
        linear_probe.main(["--config", str(tmp_path / "cfg.yaml"), "--checkpoint", "random", "--synthetic_images", "64", "--batch_size", "32",
                           "--max_epochs", "1", "--resume", str(tmp_path / "bad.pt")])
    assert str(e.value).startswith("linear_probe: --resume: mu has ")
    assert not (tmp_path / "outputs").exists()                   # refused before anything is written


def test_attentive_probe_resume_refusal_names_the_flag(dev, tmp_path):
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe
    from tests.test_gpu_attentive_probe import run_cli
    state = AttentiveProbe(64, 10, 4).state_dict()
    state["dim"] = 128
    torch.save(dict(probe=state, best=None, epoch=1), tmp_path / "bad.pt")
    with pytest.raises(SystemExit) as e:
        run_cli(tmp_path, "bad", "--max_epochs", "1", "--resume", str(tmp_path / "bad.pt"))
    assert str(e.value).startswith("attentive_probe: --resume: the state has dim = 128")
    assert not (tmp_path / "bad").exists()
