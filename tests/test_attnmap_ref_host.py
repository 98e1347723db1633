"""The attention-map reference and its bound (tests/attnmap_ref.py) on the CPU: the row chain against the explicit rollout product,
the sums the maps must have, one-hot weights, the bound's sanity, mutations of the reference that the bound must catch, the case
table's coverage, the oracle walk, ``attention_grid`` and the argument checks of scripts/evaluation/visualize_attention.py."""
import argparse
import dataclasses
import math

import pytest
import torch

from oracle import mae_oracle as O
from tests import attnmap_ref as R
from tests.attn_ref import split_heads

SMALL = [R.Case("f32", 2, 17, 3, 24), R.Case("bf16", 3, 5, 2, 16), R.Case("f32", 1, 1, 1, 32), R.Case("bf16", 2, 65, 2, 64)]
TD = {"f32": torch.float32, "bf16": torch.bfloat16}


def blocks_of(c, n=3):
    """n independent blocks' probabilities for a case: (B, H, T, T) each."""
    return [R.probabilities(R.gen_qkv(dataclasses.replace(c, B=c.B + i), "random", TD[c.dtype])[:c.B], c.H, c.hd)[1] for i in range(n)]


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_chain_is_a_row_of_the_explicit_product(c):
    Ps = blocks_of(c)
    for top in range(len(Ps)):
        M = R.rollout_matrix(Ps, top)                                   # (B, T, T)
        for row in {0, c.T - 1, c.T // 2}:
            w = torch.zeros(c.B, c.T, dtype=torch.float64)
            w[:, row] = 1.0
            got = R.rollout_ref(Ps, w, top)
            assert float((got - M[:, row]).abs().max()) <= 4e-16, (top, row)
        w = R.start_weight("mean", c.B, c.T)
        assert float((R.rollout_ref(Ps, w, top) - torch.einsum("bt,btj->bj", w, M)).abs().max()) <= 4e-16


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_sums(c):
    qkv = R.gen_qkv(c, "random", TD[c.dtype])
    for name, w in R.gen_weights(c).items():
        ph = R.colsum_ref(qkv, w, c.H, c.hd)
        assert ph.shape == (c.B, c.H, c.T)
        assert float((ph.sum(-1) - w.double().sum(-1)[:, None]).abs().max()) <= 1e-14 * max(1.0, float(w.sum(-1).max())), name
        mixed = R.mixed_ref(w, ph)
        assert float((mixed.sum(-1) - w.double().sum(-1)).abs().max()) <= 1e-14 * max(1.0, float(w.sum(-1).max())), name
    Ps = blocks_of(c)
    for q in ("cls", "mean"):
        r = R.rollout_ref(Ps, R.start_weight(q, c.B, c.T))
        assert float((r.sum(-1) - 1).abs().max()) <= 1e-14 and bool((r >= 0).all())


@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_one_hot_weight_returns_a_row_of_P(c):
    qkv = R.gen_qkv(c, "random", TD[c.dtype])
    P = R.probabilities(qkv, c.H, c.hd)[1]
    ws = R.gen_weights(c)
    assert torch.equal(R.colsum_ref(qkv, ws["onehot_first"], c.H, c.hd), P[:, :, 0])
    assert torch.equal(R.colsum_ref(qkv, ws["onehot_last"], c.H, c.hd), P[:, :, c.T - 1])
    # and against the softmax of torch, from the same split
    q, k, _ = (x.double() for x in split_heads(qkv, c.H, c.hd, 3))
    ref = torch.softmax(c.hd ** -0.5 * (q @ k.transpose(-1, -2)), -1)
    assert float((P - ref).abs().max()) <= 1e-15


@pytest.mark.parametrize("family", ["random", "large"])
@pytest.mark.parametrize("c", SMALL, ids=lambda c: c.id)
def test_bound_is_positive_finite_and_small(c, family):
    qkv = R.gen_qkv(c, family, TD[c.dtype])
    for name, w in R.gen_weights(c).items():
        e_head, e_mixed = R.colsum_bound(qkv, w, c.H, c.hd)
        for e in (e_head, e_mixed):
            assert bool(torch.isfinite(e).all()) and bool((e > 0).all()), name
        # a first-order bound of an fp32 computation, relative to the quantity's own size (sum w): about 2 (hd + 3) u A, with
        # A = scale sum_d |q k| near 0.64 sqrt(hd) <= 5 at sigma = 1 and 256 times that at sigma = 16
        cap = 1e-4 if family == "random" else 5e-2
        assert float(e_head.max()) <= cap * max(float(w.sum(-1).max()), 1e-30) + 1e-30, (name, float(e_head.max()))
    if family == "large" and c.T >= 17:
        assert float(R.probabilities(qkv, c.H, c.hd)[0].abs().max()) > 100.0


def _mutants(c, qkv, w):
    """References with one thing wrong each -> {name: per_head, mixed}."""
    S, P, _ = R.probabilities(qkv, c.H, c.hd)
    out = {}
    Pn = torch.softmax(S * c.hd ** 0.5, -1)                                # the scale dropped
    out["no scale"] = (R.colsum_from(Pn, w), R.mixed_ref(w, R.colsum_from(Pn, w)))
    Pk = P.clone()                                                         # one key shifted by one: columns j and j + 1 trade places
    j = c.T // 3
    Pk[..., [j, j + 1]] = P[..., [j + 1, j]]
    out["key shift"] = (R.colsum_from(Pk, w), R.mixed_ref(w, R.colsum_from(Pk, w)))
    ph = R.colsum_from(P, w)
    if c.H > 1:                                                            # the head mean over H - 1 heads
        out["H - 1 heads"] = (None, 0.5 * w.double() + 0.5 * ph[:, :-1].mean(1))
    return out


@pytest.mark.parametrize("c", [c for c in SMALL if c.T >= 5], ids=lambda c: c.id)
def test_mutations_exceed_the_bound(c):
    qkv = R.gen_qkv(c, "random", TD[c.dtype])
    for name, w in R.gen_weights(c).items():
        parts = R.probabilities(qkv, c.H, c.hd)
        ph = R.colsum_from(parts[1], w)
        mixed = R.mixed_ref(w, ph)
        e_head, e_mixed = R.colsum_bound(qkv, w, c.H, c.hd, parts)
        # the unmutated reference rounded to fp32 passes: the bound leaves room for the output's own rounding
        assert bool(((ph.float().double() - ph).abs() <= e_head).all()) and bool(((mixed.float().double() - mixed).abs() <= e_mixed).all())
        for mname, (mph, mmixed) in _mutants(c, qkv, w).items():
            if mph is not None:
                assert float(((mph - ph).abs() / e_head).max()) > 100.0, (name, mname)
            assert float(((mmixed - mixed).abs() / e_mixed).max()) > 100.0, (name, mname)


def test_case_table_covers_every_pair():
    table = R.cases(512)
    assert 30 <= len(table) <= 40 and len({c.id for c in table}) == len(table)
    assert R.uncovered(table, 512) == []
    assert {c.T for c in table} == set(R.TS) | {512}
    assert all(sum(c.T == T for c in table) == 3 for T in R.TS)
    assert {c.route for c in table} == {f"{d}/NK{n}" for d in R.DTYPES for n in (1, 2, 3, 4, 5, 8)}
    assert any(c.T >= 128 and c.H >= 3 for c in table) and any(c.T >= 128 and c.B >= 3 for c in table)
    for c in table[:6]:
        ws = R.gen_weights(c)
        assert all(w.shape == (c.B, c.T) and w.dtype == torch.float32 and bool((w >= 0).all()) for w in ws.values())
        assert bool((ws["sparse"] == 0).any(dim=1).all())


def test_oracle_walk_matches_the_oracle_and_its_fp64_form():
    cfg = O.MAEConfig(image_size=32, patch_size=8, in_chans=3, embed_dim=48, depth=3, num_heads=2, decoder_embed_dim=64, decoder_depth=1,
                      decoder_num_heads=2)
    params = O.init_params(cfg, 73)
    O.randomize_params(params, seed=5)
    imgs = O.synthetic_images(3, cfg, seed=4)
    with torch.no_grad():
        for with_cls in (True, False):
            T = cfg.sequence_length - (0 if with_cls else 1)
            Ps = R.oracle_walk(params, cfg, imgs, with_cls, False)
            P64 = R.walk_fp64(params, cfg, imgs, with_cls)
            Pb = R.oracle_walk(params, cfg, imgs, with_cls, True)
            assert len(Ps) == cfg.depth and all(p.shape == (3, 2, T, T) for p in Ps + P64 + Pb)
            assert P64[0].dtype == torch.float64 and Ps[0].dtype == torch.float32
            assert float((Ps[-1].double() - P64[-1]).abs().max()) < 1e-5 and 1e-5 < float((Pb[-1].double() - P64[-1]).abs().max()) < 5e-2
            assert float((P64[-1].sum(-1) - 1).abs().max()) < 1e-14
        # the walk's residual stream is the oracle's: one more block changes nothing before it
        short = R.oracle_walk(params, dataclasses.replace(cfg, depth=2), imgs, True, False)
        full = R.oracle_walk(params, cfg, imgs, True, False)
        assert all(torch.equal(a, b) for a, b in zip(short, full))
        P64 = R.walk_fp64(params, cfg, imgs, True)
        m = R.maps_of(P64, "cls", [0, 2])
        assert m.shape == (3, 2, 2, cfg.sequence_length) and torch.equal(m[:, 1], P64[2][:, :, 0])


# ------------------------------------------------------------------------------------------------ attention_grid, CLI arguments
def test_attention_grid():
    from ssrl_vit_mae_jepa_amd.representation import attention_grid
    g = torch.Generator().manual_seed(3)
    maps = torch.rand(2, 3, 4, 17, generator=g)
    maps = maps / maps.sum(-1, keepdim=True)
    out = attention_grid(maps, True, 4)
    assert out.shape == (2, 3, 4, 4, 4)
    assert torch.allclose(out.sum((-1, -2)), torch.ones(2, 3, 4))
    assert torch.allclose(out.flatten(-2), maps[..., 1:] / maps[..., 1:].sum(-1, keepdim=True))
    assert float(out[0, 0, 0, 1, 2]) == pytest.approx(float(maps[0, 0, 0, 1 + 4 + 2] / maps[0, 0, 0, 1:].sum()))   # row-major patches
    roll = maps[:, 0, 0, 1:]
    out = attention_grid(roll, False, 4)
    assert out.shape == (2, 4, 4) and torch.allclose(out.flatten(-2), roll / roll.sum(-1, keepdim=True))
    for bad, wc, grid in ((maps, False, 4), (maps, True, 3), (maps[..., :16], True, 4)):
        with pytest.raises(ValueError):
            attention_grid(bad, wc, grid)
    only_cls = torch.zeros(1, 17)
    only_cls[0, 0] = 1.0
    with pytest.raises(ValueError):
        attention_grid(only_cls, True, 4)


def test_cli_arguments_and_stats():
    from scripts.evaluation import visualize_attention as V
    mae_cfg = dict(encoder=dict(embed_dim=48, depth=4, num_heads=2))
    jepa_cfg = dict(mae_cfg, predictor=dict(pred_embed_dim=32))
    a = V.parse_args(["--checkpoint", "random"])
    assert (a.layers, a.query, a.rollout, a.num_samples, a.encoder) == ("last", None, False, 8, "target")
    assert V.resolve_request(a, mae_cfg) == ((3,), "cls")
    assert V.resolve_request(a, jepa_cfg) == ((3,), "mean")
    a = V.parse_args(["--checkpoint", "x.ckpt", "--layers", "each", "--query", "mean", "--rollout", "--num_samples", "4", "--synthetic_images", "16"])
    assert V.resolve_request(a, mae_cfg) == ((0, 1, 2, 3), "mean") and a.rollout and a.synthetic_images == 16
    assert V.resolve_request(V.parse_args(["--checkpoint", "random", "--layers", "1,-1"]), mae_cfg)[0] == (1, 3)
    for argv, cfg in ((["--checkpoint", "random", "--layers", "7"], mae_cfg), (["--checkpoint", "random", "--layers", "last9"], mae_cfg),
                      (["--checkpoint", "random", "--layers", "1,1"], mae_cfg), (["--checkpoint", "random", "--query", "cls"], jepa_cfg),
                      (["--checkpoint", "random", "--num_samples", "0"], mae_cfg), (["--checkpoint", "random", "--synthetic_images", "0"], mae_cfg)):
        with pytest.raises(SystemExit):
            V.resolve_request(V.parse_args(argv), cfg)
    with pytest.raises(SystemExit):
        V.parse_args(["--checkpoint", "random", "--query", "max"])
    with pytest.raises(SystemExit):
        V.parse_args([])
    # the statistics: a uniform map has entropy ln T, a one-hot map 0 and all its mass where it points
    T = 17
    maps = torch.full((5, 2, 3, T), 1.0 / T)
    maps[:, 1, 2] = 0.0
    maps[:, 1, 2, 0] = 1.0
    s = V.attention_stats(maps, (1, 3), True)
    assert s["tokens"] == T and s["uniform_entropy"] == pytest.approx(math.log(T)) and set(s["blocks"]) == {"1", "3"}
    assert s["blocks"]["1"]["entropy"] == pytest.approx([math.log(T)] * 3) and s["blocks"]["1"]["class_mass"] == pytest.approx([1 / T] * 3)
    assert s["blocks"]["3"]["entropy"][2] == pytest.approx(0.0, abs=1e-12) and s["blocks"]["3"]["class_mass"][2] == pytest.approx(1.0)
    assert V.attention_stats(maps, (1, 3), False)["blocks"]["3"]["class_mass"] == [0.0, 0.0, 0.0]
    with pytest.raises(ValueError):
        V.attention_stats(maps, (1,), True)
    assert isinstance(a, argparse.Namespace)


def test_figure_writer(tmp_path):
    from scripts.evaluation.visualize_attention import save_attention_figure
    g = torch.Generator().manual_seed(1)
    imgs = torch.randint(0, 256, (2, 3, 32, 32), dtype=torch.uint8, generator=g)
    grids = torch.rand(2, 2, 4, 4, generator=g)
    p = save_attention_figure(imgs, grids, torch.rand(2, 4, 4, generator=g), tmp_path / "a" / "fig.png", "title")
    assert p.exists() and p.stat().st_size > 1000
    assert save_attention_figure(imgs, grids, None, tmp_path / "b.png").exists()
    with pytest.raises(ValueError):
        save_attention_figure(imgs.float(), grids, None, tmp_path / "c.png")
