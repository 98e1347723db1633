"""What the probe tools share (scripts/evaluation/_probe_cli.py) and the one block parser behind ``parse_probe`` and
``parse_attentive_probe``, without a GPU: the split evaluation and the inner step loop on stubs, the epoch's batches, the parser's
refusals by their texts."""
import numpy as np
import pytest
import torch

from scripts.evaluation import _probe_cli as C


class StubProbe:
    """``evaluate`` hands out the chosen per-batch (loss (G,), correct (G,)) in turn and notes the rows it was given."""

    def __init__(self, losses, corrects):
        self.losses, self.corrects, self.rows = losses, corrects, []

    def evaluate(self, x, y):
        assert x.shape[0] == y.shape[0]
        i = len(self.rows)
        self.rows.append(x[:, 0].tolist())
        return None, torch.tensor(self.losses[i], dtype=torch.float32), torch.tensor(self.corrects[i], dtype=torch.int32)


@pytest.mark.parametrize("losses,corrects", [([[0.5], [0.25], [2.0]], [[2], [1], [1]]),
                                             ([[0.5, 1.5, 0.125], [0.25, 3.0, 8.0], [2.0, 0.75, 1.0]], [[2, 0, 3], [1, 3, 0], [1, 0, 1]])])
def test_evaluate_split_is_the_row_weighted_mean(losses, corrects):
    x, y = torch.arange(7.0).view(7, 1), torch.zeros(7, dtype=torch.int64)
    probe = StubProbe(losses, corrects)
    loss, acc = C.evaluate_split(probe, x, y, 3)
    assert probe.rows == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0]]                       # batches of 3, 3 and 1 rows, in order
    rows = np.array([3, 3, 1], dtype=np.float64)
    want_loss = (np.array(losses, dtype=np.float64) * rows[:, None]).sum(0) / 7           # every product and sum is exact in float64
    want_acc = np.array(corrects, dtype=np.float64).sum(0) / 7
    assert loss == want_loss.tolist() and acc == want_acc.tolist()
    assert all(type(v) is float for v in loss + acc)


@pytest.mark.parametrize("G", [1, 3])
def test_run_steps_sums_and_order(G):
    n, batch = 7, 3
    x, y = torch.arange(float(n)).view(n, 1) * 10, torch.arange(n)
    batches = C.epoch_batches(n, batch, 73, 0)
    calls, gathered = [], []

    def gather(i, j):
        gathered.append(i)
        assert j.dtype == torch.int64 and j.device.type == "cpu"
        return x[j], y[j]

    def step(inputs, labels):
        k = len(calls)
        calls.append((inputs[:, 0].tolist(), labels.tolist()))
        return torch.full((G,), 0.5 * (k + 1), dtype=torch.float32) * torch.arange(1, G + 1), torch.arange(G, dtype=torch.int32) + k

    loss_sum, correct_sum, rows, seconds = C.run_steps(batches, gather, step, torch.device("cpu"))
    assert gathered == [0, 1, 2] and rows == n and seconds >= 0.0
    assert calls == [((x[torch.from_numpy(b), 0]).tolist(), b.tolist()) for b in batches]   # one step per batch, in epoch_batches' order
    lens = [len(b) for b in batches]
    assert loss_sum.dtype == torch.float64 and correct_sum.dtype == torch.int64
    assert loss_sum.tolist() == [sum(0.5 * (k + 1) * (g + 1) * lens[k] for k in range(3)) for g in range(G)]
    assert correct_sum.tolist() == [sum(g + k for k in range(3)) for g in range(G)]


def test_epoch_batches_min_rows():
    from scripts.evaluation import attentive_probe, linear_probe
    order = np.random.default_rng([73, 4]).permutation(65)          # the shuffle of (seed, epoch) both tools have always drawn
    two, one = C.epoch_batches(65, 32, 73, 4, min_rows=2), C.epoch_batches(65, 32, 73, 4, min_rows=1)
    assert [len(b) for b in two] == [32, 32] and [len(b) for b in one] == [32, 32, 1]
    assert np.array_equal(np.concatenate(one), order) and np.array_equal(np.concatenate(two), order[:64])
    for mine, theirs in ((two, linear_probe.epoch_batches(65, 32, 73, 4)), (one, attentive_probe.epoch_batches(65, 32, 73, 4))):
        assert len(mine) == len(theirs) and all(np.array_equal(a, b) for a, b in zip(mine, theirs))
    assert [len(b) for b in C.epoch_batches(66, 32, 73, 0, min_rows=2)] == [32, 32, 2]


def test_block_parser_refusals_and_casts():
    from ssrl_vit_mae_jepa_amd.attentive import ATTENTIVE_DEFAULTS, attentive_lr, parse_attentive_probe
    from ssrl_vit_mae_jepa_amd.probe import PROBE_DEFAULTS, parse_block, parse_probe, probe_lr
    for parse, name, defaults in ((parse_probe, "probe", PROBE_DEFAULTS), (parse_attentive_probe, "attentive_probe", ATTENTIVE_DEFAULTS)):
        with pytest.raises(ValueError) as e:
            parse([1, 2])
        assert str(e.value) == f"{name} must be a mapping, got [1, 2]"
        with pytest.raises(ValueError) as e:
            parse(dict(zeta=1, alpha=2, batch_size=8))
        assert str(e.value) == f"{name}: unknown keys ['alpha', 'zeta']"
        out = parse(dict(batch_size="32", weight_decay=None, total_epochs=7.0, bn_eps="1e-5"))
        assert out["batch_size"] == 32 and type(out["batch_size"]) is int and type(out["total_epochs"]) is int
        assert out["weight_decay"] == defaults["weight_decay"] and out["bn_eps"] == 1e-5
        assert parse({}) == parse(None) == defaults and parse(None) is not defaults
    assert parse_block(dict(a="3", b=None), dict(a=1, b=2.5, c="x"), "blk", ("a",), ("b",)) == dict(a=3, b=2.5, c="x")
    assert attentive_lr is probe_lr
