"""AttentiveProbe on the MI355X: one step against the fp64 reference of tests/attnpool_ref.py at the project's fp32 parity tolerances
(DESIGN.md 9), evaluation mode against the running-statistics form, a state-dict round trip, the probe learning where to look, and
the command-line tool (two epochs on synthetic images, resumed bit for bit)."""
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import attnpool_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]

LOSS_TOL, GRAD_TOL, LOGIT_TOL = 1e-4, 3e-4, 1e-4   # loss relative, each gradient tensor in relative norm, logits


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return torch.device("cuda", 0)


def relnorm(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def make_probe(dev, D, C, H, seed=5, wd=0.05):
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe
    probe = AttentiveProbe(D, C, H, dict(weight_decay=wd), seed=seed)
    r = torch.Generator().manual_seed(seed + 1)
    # larger weights than the init: a peaked softmax and gradients of a comparable size in every tensor
    probe.q.copy_(torch.randn(D, generator=r))
    probe.wk.copy_(torch.randn(D, D, generator=r) * (2.0 / D ** 0.5))
    probe.wv.copy_(torch.randn(D, D, generator=r) / D ** 0.5)
    probe.w.copy_(torch.randn(C, D, generator=r) * 0.3)
    probe.b.copy_(torch.randn(C, generator=r) * 0.1)
    return probe.to(dev)


def params(probe):
    return {k: getattr(probe, k).detach().cpu().numpy().copy() for k in ("q", "wk", "wv", "w", "b")}


@pytest.mark.parametrize("B,T,D,H,C", [(6, 37, 64, 4, 10), (3, 145, 384, 6, 10)])
def test_one_step_against_the_fp64_reference(dev, B, T, D, H, C):
    x = R.gen_case(B, T, D, H, seed=1)["x"]
    labels = np.random.default_rng([B, T, 3]).integers(0, C, B)
    probe = make_probe(dev, D, C, H)
    p0 = params(probe)
    ref = R.definition(x, p0["q"], p0["wk"], p0["wv"], p0["w"], p0["b"], labels, H, eps=probe.cfg["bn_eps"])
    xd, yd = torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev)
    loss, correct = probe.loss_and_grads(xd, yd)
    torch.cuda.synchronize()
    logits = probe.last["logits"].cpu().numpy()
    rl = abs(float(loss) - float(ref["loss"])) / abs(float(ref["loss"]))
    rg = relnorm(logits, ref["logits"])
    print(f"{B}x{T}x{D} H{H}: loss rel {rl:.3g}, logits rel norm {rg:.3g}")
    fails = []
    if not rl <= LOSS_TOL:
        fails.append(f"loss {float(loss)!r} vs {float(ref['loss'])!r}: rel {rl:.3g}")
    if not rg <= LOGIT_TOL:
        fails.append(f"logits: relative norm {rg:.3g}")
    for name, key in (("q", "dq"), ("wk", "dwk"), ("wv", "dwv"), ("w", "dw"), ("b", "db")):
        r = relnorm(probe.grad(name).cpu().numpy(), ref[key])
        print(f"{B}x{T}x{D} H{H}: d{name} rel norm {r:.3g}")
        if not r <= GRAD_TOL:
            fails.append(f"d{name}: relative norm {r:.3g}")
    assert int(correct) == int((ref["logits"].argmax(1) == labels).sum())
    # the running statistics after one training-mode call: torch's BatchNorm1d update (momentum 0.1, the unbiased variance)
    n = B * T
    assert relnorm(probe.running_mean.cpu().numpy(), 0.1 * ref["mu"]) <= 1e-5
    assert relnorm(probe.running_var.cpu().numpy(), 0.9 + 0.1 * ref["var"] * n / (n - 1)) <= 1e-5
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("B,T,D,H,C", [(6, 37, 64, 4, 10)])
def test_evaluation_uses_the_running_statistics(dev, B, T, D, H, C):
    x = R.gen_case(B, T, D, H, seed=2)["x"]
    labels = np.random.default_rng([B, T, 4]).integers(0, C, B)
    probe = make_probe(dev, D, C, H)
    r = np.random.default_rng(8)
    rm, rv = r.standard_normal(D).astype(np.float32), (0.5 + r.random(D)).astype(np.float32)
    probe.running_mean.copy_(torch.from_numpy(rm))
    probe.running_var.copy_(torch.from_numpy(rv))
    p0 = params(probe)
    before = probe.state_dict()
    logits, loss, correct = probe.evaluate(torch.from_numpy(x).to(dev), torch.from_numpy(labels).to(dev))
    torch.cuda.synchronize()
    ref = R.definition(x, p0["q"], p0["wk"], p0["wv"], p0["w"], p0["b"], labels, H, eps=probe.cfg["bn_eps"], stats=(rm, rv))
    assert relnorm(logits.cpu().numpy(), ref["logits"]) <= LOGIT_TOL
    assert abs(float(loss) - float(ref["loss"])) <= LOSS_TOL * abs(float(ref["loss"]))
    assert int(correct) == int((ref["logits"].argmax(1) == labels).sum())
    after = probe.state_dict()
    for k in ("flat", "exp_avg", "exp_avg_sq", "running_mean", "running_var"):
        assert torch.equal(before[k], after[k]), k                                             # evaluation changes no state
    single, _, _ = probe.evaluate(torch.from_numpy(x[:1]).to(dev))                             # one image is enough in evaluation
    assert torch.equal(single.cpu(), logits[:1].cpu())


def test_state_dict_round_trip_reproduces_the_next_step(dev):
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe
    B, T, D, H, C = 6, 37, 64, 4, 10
    x = torch.from_numpy(R.gen_case(B, T, D, H, seed=3)["x"]).to(dev)
    y = torch.from_numpy(np.random.default_rng(6).integers(0, C, B)).to(dev)
    a = make_probe(dev, D, C, H)
    a.step(x, y, 1e-3)
    a.step(x, y, 1e-3)
    state = a.state_dict()
    b = AttentiveProbe(D, C, H, dict(weight_decay=0.05), seed=11).to(dev)
    b.load_state_dict(state)
    la, _ = a.step(x, y, 1e-3)
    lb, _ = b.step(x, y, 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(la.cpu(), lb.cpu()) and a.steps == b.steps == 3
    sa, sb = a.state_dict(), b.state_dict()
    for k in ("flat", "exp_avg", "exp_avg_sq", "running_mean", "running_var"):
        assert torch.equal(sa[k], sb[k]), k
    wd0 = make_probe(dev, D, C, H, wd=0.0)
    wd1 = make_probe(dev, D, C, H, wd=0.5)
    wd0.step(x, y, 1e-3); wd1.step(x, y, 1e-3)
    torch.cuda.synchronize()
    assert torch.equal(wd0.q.cpu(), wd1.q.cpu()) and torch.equal(wd0.b.cpu(), wd1.b.cpu())     # weight decay reaches the three matrices only
    assert not torch.equal(wd0.wk.cpu(), wd1.wk.cpu()) and not torch.equal(wd0.wv.cpu(), wd1.wv.cpu()) and not torch.equal(wd0.w.cpu(), wd1.w.cpu())


# ------------------------------------------------------------------------------------------------------------------
# learns where to look
# ------------------------------------------------------------------------------------------------------------------
LEARN = dict(T=64, D=32, H=4, C=4, n=512, steps=100, lr=1e-2)
REFERENCE_ACCURACY = 0.89453125     # torch fp32 on the CPU with the generators below (reference_accuracies)
MEAN_POOL_ACCURACY = 0.326171875       # BatchNorm + mean-pool linear probe, same data and steps (chance 0.25)


def learn_data():
    """Unit-noise tokens; one randomly placed token per image carries a class prototype (norm 3) plus a shared marker (norm 4)."""
    T, D, C, n = LEARN["T"], LEARN["D"], LEARN["C"], LEARN["n"]
    g = torch.Generator().manual_seed(1)
    proto = torch.randn(C, D, generator=g)
    proto = 3 * proto / proto.norm(dim=1, keepdim=True)
    marker = torch.randn(D, generator=g)
    marker = 4 * marker / marker.norm()

    def make(seed):
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(n, T, D, generator=g)
        y = torch.randint(0, C, (n,), generator=g)
        pos = torch.randint(0, T, (n,), generator=g)
        x[torch.arange(n), pos] += proto[y] + marker
        return x, y
    return make(2), make(3)


def learn_init():
    """The probe the GPU run starts from: AttentiveProbe's own initialisation (seed 5), no weight decay."""
    from ssrl_vit_mae_jepa_amd.attentive import AttentiveProbe
    return AttentiveProbe(LEARN["D"], LEARN["C"], LEARN["H"], dict(weight_decay=0.0), seed=5)


def reference_accuracies():
    """(attentive, mean-pool) test accuracies of the torch fp32 CPU reference: 100 full-batch AdamW steps at lr 1e-2 from learn_init's
    parameters, the training set's statistics in the BatchNorm."""
    (xtr, ytr), (xte, yte) = learn_data()
    T, D, H, C = LEARN["T"], LEARN["D"], LEARN["H"], LEARN["C"]
    hd = D // H
    mu = xtr.reshape(-1, D).mean(0)
    r = (xtr.reshape(-1, D).var(0, unbiased=False) + 1e-6).rsqrt()
    out = []
    for attentive in (True, False):
        init = learn_init()
        q, wk, wv, w, b = (getattr(init, k).clone().requires_grad_() for k in ("q", "wk", "wv", "w", "b"))
        opt = torch.optim.AdamW([q, wk, wv, w, b] if attentive else [w, b], lr=LEARN["lr"], weight_decay=0.0)

        def fwd(x):
            xh = (x - mu) * r
            if not attentive:
                return xh.mean(1) @ w.T + b
            n = x.shape[0]
            k = (xh @ wk.T).reshape(n, T, H, hd)
            v = (xh @ wv.T).reshape(n, T, H, hd)
            a = (torch.einsum("hj,bthj->bth", q.reshape(H, hd), k) * hd ** -0.5).softmax(1)
            return torch.einsum("bth,bthj->bhj", a, v).reshape(n, D) @ w.T + b
        for _ in range(LEARN["steps"]):
            loss = torch.nn.functional.cross_entropy(fwd(xtr), ytr)
            opt.zero_grad()
            loss.backward()
            opt.step()
        with torch.no_grad():
            out.append(float((fwd(xte).argmax(1) == yte).float().mean()))
    return tuple(out)


def test_learns_where_to_look(dev):
    """The recipe of the issue's CPU experiment: 64 x 32 tokens, 4 classes, 512 + 512 images, 100 full-batch steps at lr 1e-2, no weight
    decay.  With the generators of learn_data and the initialisation of learn_init the torch fp32 reference on the CPU reaches 0.8945
    test accuracy and the BatchNorm + mean-pool linear probe 0.3262 (the acceptance conditions on the inputs: at least 0.8, at most
    0.45).  The GPU run must reach the recorded reference value minus 0.05; the margin covers fp32 summation-order differences over 100
    steps and the running statistics the GPU evaluates with (the reference keeps the training set's)."""
    assert REFERENCE_ACCURACY >= 0.8 and MEAN_POOL_ACCURACY <= 0.45
    (xtr, ytr), (xte, yte) = learn_data()
    probe = learn_init().to(dev)
    xtr, ytr, xte, yte = (t.to(dev) for t in (xtr, ytr, xte, yte))
    for _ in range(LEARN["steps"]):
        loss, _ = probe.step(xtr, ytr, LEARN["lr"])
    _, _, correct = probe.evaluate(xte, yte)
    acc = int(correct) / LEARN["n"]
    print(f"attentive probe on the GPU: final loss {float(loss):.4f}, test accuracy {acc:.4f} (reference {REFERENCE_ACCURACY:.4f}, mean pool {MEAN_POOL_ACCURACY:.4f})")
    assert acc >= REFERENCE_ACCURACY - 0.05


# ------------------------------------------------------------------------------------------------------------------
# the command-line tool
# ------------------------------------------------------------------------------------------------------------------
TINY_MODEL = dict(general=dict(image_size=32, patch_size=8, in_chans=3, loss="mse", num_target_blocks=2, target_scale=[0.15, 0.2],
                               target_aspect=[0.75, 1.5], context_scale=[0.85, 1.0]),
                  encoder=dict(embed_dim=64, depth=2, num_heads=4), predictor=dict(pred_embed_dim=64, pred_depth=1, pred_num_heads=4),
                  head=dict(embed_dim=64, pool="mean_patches"))


def run_cli(tmp_path, name, *extra):
    """attentive_probe --checkpoint random --synthetic_images 200 on the repository's config shrunk to a 2-block, 64-wide encoder."""
    import yaml
    from scripts.evaluation import attentive_probe
    cfg = yaml.safe_load((ROOT / "configs" / "ijepa_vits8_attnprobe.yaml").read_text())
    cfg["model"] = TINY_MODEL
    cfg["engine"] = dict(precision="fp32")
    cfg["attentive_probe"] = dict(cfg["attentive_probe"], batch_size=64)
    cfg_path = tmp_path / "cfg.yaml"
    cfg_path.write_text(yaml.safe_dump(cfg))
    return attentive_probe.main(["--config", str(cfg_path), "--checkpoint", "random", "--synthetic_images", "200", "--output_dir", str(tmp_path / name), *extra])


def test_cli_two_epochs_and_resume(dev, tmp_path):
    res = run_cli(tmp_path, "full", "--max_epochs", "2")
    assert res["epochs"] == 2 and res["heads"] == 4 and res["tokens_per_image"] == 16 and 0.0 <= res["val_acc"] <= 1.0 and 0.0 <= res["test_acc"] <= 1.0
    last = torch.load(tmp_path / "full" / "attnprobe_last.pt", map_location="cpu", weights_only=False)
    assert last["epoch"] == 2 and (tmp_path / "full" / "attnprobe_best.pt").exists() and (tmp_path / "full" / "attnprobe.json").exists()
    run_cli(tmp_path, "part", "--max_epochs", "1")
    run_cli(tmp_path, "part", "--max_epochs", "1", "--resume", str(tmp_path / "part" / "attnprobe_last.pt"))
    again = torch.load(tmp_path / "part" / "attnprobe_last.pt", map_location="cpu", weights_only=False)
    assert again["epoch"] == 2 and last["probe"]["steps"] == again["probe"]["steps"]
    for k in ("flat", "exp_avg", "exp_avg_sq", "running_mean", "running_var"):
        assert torch.equal(last["probe"][k], again["probe"][k]), k                             # resumed: the same bits as uninterrupted
