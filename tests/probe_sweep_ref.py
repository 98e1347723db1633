"""float64 restatement of the linear-probe sweep (k_probe_sweep.hip, probe.ProbeSweep) for the tests, built on tests/probe_ref.py: a
sweep is G independent probes that share their BatchNorm, so every piece is probe_ref's per head.

  head_floats   HF = round_up(C D + C, 4): one head's segment [W (C, D) | b (C) | zero padding] of the stacked buffer
  pack / unpack the stacked (G, HF) buffer from and to per-head (W, b)
  sweep_head    probe_ref.head per head on the same rows
  sweep_step    one ProbeSweep.step: bn_train once, then per head probe_ref.head and lars_step on W (adapt 1, the head's lr and
                weight decay) and on b (adapt 0); the per-head lr is the fp32 value the kernel receives
  gen_heads     G differing heads of std 0.01, biases of the same size
  gen_rows      gen_bn rows passed through bn_train: what the head sees in a step
"""
from __future__ import annotations

import numpy as np

from tests import probe_ref as R

F = np.float32


def head_floats(C: int, D: int) -> int:
    return (C * D + C + 3) // 4 * 4


def pack(weights, biases) -> np.ndarray:
    G, (C, D) = len(weights), np.asarray(weights[0]).shape
    out = np.zeros((G, head_floats(C, D)), dtype=F)
    for g in range(G):
        out[g, :C * D] = np.asarray(weights[g], dtype=F).reshape(-1)
        out[g, C * D:C * D + C] = np.asarray(biases[g], dtype=F)
    return out


def unpack(flat, C: int, D: int):
    flat = np.asarray(flat)
    return [flat[g, :C * D].reshape(C, D) for g in range(flat.shape[0])], [flat[g, C * D:C * D + C] for g in range(flat.shape[0])]


def gen_heads(G: int, C: int, D: int, seed: int = 0):
    r = np.random.default_rng([G, C, D, seed, 17])
    return [(0.01 * r.standard_normal((C, D))).astype(F) for _ in range(G)], [(0.01 * r.standard_normal(C)).astype(F) for _ in range(G)]


def gen_rows(B: int, D: int, seed: int = 0) -> np.ndarray:
    """(B, D) fp32 normalised rows: gen_bn through bn_train (one row: the raw row, BatchNorm needs two)."""
    x = R.gen_bn(B, D, seed)
    return x if B < 2 else R.bn_train(x)["y"].astype(F)


def sweep_head(y, weights, biases, labels=None) -> list:
    return [R.head(y, w, b, labels) for w, b in zip(weights, biases)]


def head_lr(base_learning_rate: float, batch_size: int, lr_factor: float) -> float:
    """The fp32 learning rate of a head: base * batch / 256 * factor in double, rounded once."""
    return float(F(float(base_learning_rate) * int(batch_size) / 256.0 * float(lr_factor)))


def sweep_step(weights, biases, mu_w, mu_b, running_mean, running_var, feats, labels, grid, lr_factor, cfg) -> dict:
    """dict(bn, heads): heads[g] = dict(head, lars_w, lars_b, lr), probe_ref.probe_step's pieces with head g's lr and weight decay."""
    bn = R.bn_train(feats, running_mean, running_var, cfg["bn_eps"], cfg["bn_momentum"])
    heads = []
    for g, hp in enumerate(grid):
        lr = head_lr(hp["base_learning_rate"], cfg["batch_size"], lr_factor)
        h = R.head(bn["y"], weights[g], biases[g], labels)
        lw = R.lars_step(np.asarray(weights[g], dtype=np.float64).reshape(-1), h["dW"].reshape(-1), mu_w[g], 1, lr, cfg["momentum"],
                         hp["weight_decay"], cfg["trust_coefficient"])
        lb = R.lars_step(biases[g], h["db"], mu_b[g], 0, lr, cfg["momentum"], hp["weight_decay"], cfg["trust_coefficient"])
        heads.append(dict(head=h, lars_w=lw, lars_b=lb, lr=lr))
    return dict(bn=bn, heads=heads)
