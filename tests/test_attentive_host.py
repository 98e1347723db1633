"""The attentive probe's host side without a GPU: the YAML block and its defaults, the command line on top of it, the flat parameter
layout and the constructor's limits."""
from pathlib import Path

import pytest
import torch
import yaml

ROOT = Path(__file__).resolve().parents[1]


def test_defaults_and_parsing():
    from ssrl_vit_mae_jepa_amd.attentive import ATTENTIVE_DEFAULTS, attentive_lr, parse_attentive_probe
    d = parse_attentive_probe(None)
    assert d == ATTENTIVE_DEFAULTS
    assert (d["total_epochs"], d["warmup_epochs"], d["base_learning_rate"], d["weight_decay"], d["heads"], d["tokens"]) == (90, 10, 1e-3, 0.05, None, "patches")
    c = parse_attentive_probe(dict(batch_size="512", heads=8, weight_decay=None, tokens="all"))
    assert c["batch_size"] == 512 and c["heads"] == 8 and c["weight_decay"] == 0.05 and c["tokens"] == "all"      # a null key keeps its default
    assert attentive_lr(c) == pytest.approx(1e-3 * 512 / 256)
    for bad, word in ((dict(lr=1.0), "unknown keys"), (dict(heads=17), "heads"), (dict(tokens="cls"), "tokens"), (dict(total_epochs=0), "total_epochs"),
                      (dict(base_learning_rate=0.0), "base_learning_rate"), (dict(bn_momentum=1.5), "bn_momentum"), ([1, 2], "mapping")):
        with pytest.raises(ValueError, match=word):
            parse_attentive_probe(bad)


def test_repository_config_and_command_line():
    from scripts.evaluation import attentive_probe as cli
    from ssrl_vit_mae_jepa_amd.attentive import ATTENTIVE_DEFAULTS
    cfg = yaml.safe_load((ROOT / "configs" / "ijepa_vits8_attnprobe.yaml").read_text())
    base = yaml.safe_load((ROOT / "configs" / "ijepa_vits8.yaml").read_text())
    assert cfg["model"] == base["model"] and cfg["engine"] == base["engine"]
    args = cli.parse_args(["--checkpoint", "random"])
    assert args.encoder == "target" and args.synthetic_images is None and args.resume is None and args.max_epochs is None
    p = cli.probe_config(cfg, args)
    assert p["batch_size"] == 2000 and p["heads"] is None and p["tokens"] == "patches" and p["weight_decay"] == 0.05
    assert cli.probe_config({}, args) == ATTENTIVE_DEFAULTS                                      # no block at all: the defaults in code
    args = cli.parse_args(["--checkpoint", "random", "--encoder", "context", "--heads", "12", "--tokens", "all", "--base_learning_rate", "5e-4",
                           "--synthetic_images", "200", "--max_epochs", "2", "--resume", "x.pt"])
    p = cli.probe_config(cfg, args)
    assert (p["heads"], p["tokens"], p["base_learning_rate"], p["batch_size"]) == (12, "all", 5e-4, 2000)
    assert (args.encoder, args.synthetic_images, args.max_epochs, args.resume) == ("context", 200, 2, "x.pt")
    with pytest.raises(SystemExit):
        cli.parse_args(["--checkpoint", "random", "--tokens", "cls"])
    a, b = cli.epoch_batches(10, 4, 73, 0), cli.epoch_batches(10, 4, 73, 0)
    assert [len(x) for x in a] == [4, 4, 2] and all((x == y).all() for x, y in zip(a, b))
    assert sorted(int(i) for x in a for i in x) == list(range(10))
    assert any((x != y).any() for x, y in zip(a, cli.epoch_batches(10, 4, 73, 1)))


def test_layout_and_constructor():
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe, layout
    lay = layout(64, 10)
    assert lay["q"] == (0, 64) and lay["wk"] == (64, 4096) and lay["wv"] == (4160, 4096) and lay["w"] == (8256, 640) and lay["b"] == (8896, 10)
    assert lay["total"] == (0, 8908) and all(lay[k][0] % 4 == 0 for k in ("q", "wk", "wv", "w", "b"))
    p = AttentiveProbe(64, 10, 4, seed=3)
    assert p.flat.numel() == 8908 and p.q.shape == (64,) and p.wk.shape == (64, 64) and p.w.shape == (10, 64) and p.b.shape == (10,)
    assert p.q.data_ptr() == p.flat.data_ptr() and p.head_flat.data_ptr() == p.w.data_ptr()      # views, not copies
    assert 0.01 < float(p.wk.std()) < 0.03 and 0.005 < float(p.w.std()) < 0.015 and float(p.b.abs().max()) == 0.0
    assert torch.equal(p.flat, AttentiveProbe(64, 10, 4, seed=3).flat) and not torch.equal(p.flat, AttentiveProbe(64, 10, 4, seed=4).flat)
    q = AttentiveProbe(64, 10, 4, seed=9)
    q.load_state_dict(p.state_dict())
    assert torch.equal(q.flat, p.flat)
    for args, word in (((66, 10, 2), "multiple of 4"), ((1028, 10, 4), "multiple of 4"), ((64, 10, 3), "heads"), ((64, 10, 17), "heads"), ((64, 1, 4), "num_classes")):
        with pytest.raises(ValueError, match=word):
            AttentiveProbe(*args)
    with pytest.raises(ValueError, match="heads"):
        AttentiveProbe(64, 10, 8).load_state_dict(p.state_dict())
    with pytest.raises(RuntimeError, match="MI355X"):
        p.step(torch.zeros(2, 3, 64), torch.zeros(2, dtype=torch.int64), 1e-3)
