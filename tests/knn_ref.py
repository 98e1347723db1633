"""fp64 references of the k-NN probe (mae_knn_topk / mae_knn_vote) and of pooled features, for the GPU tests."""
import torch


def topk_ref(queries: torch.Tensor, bank: torch.Tensor):
    """fp64 similarities (Q, N) and the per-pair error bound D * 2^-24 * sum_d |q_d b_d| of an fp32 fma chain."""
    q, b = queries.double().cpu(), bank.double().cpu()
    return q @ b.T, q.shape[1] * 2.0 ** -24 * (q.abs() @ b.abs().T)


def check_topk(sims, idx, ref_sim, bound, k):
    """Rows sorted; every returned sim within its pair's bound of fp64; the index set equal to the fp64 top-k except for
    entries within twice the bound of the k-th value."""
    sims, idx = sims.double().cpu(), idx.cpu()
    Q = sims.shape[0]
    assert sims.shape == (Q, k) and idx.shape == (Q, k)
    d = sims[:, 1:] - sims[:, :-1]
    assert (d <= 0).all(), "rows not sorted by similarity"
    tie = d == 0
    assert (idx[:, 1:][tie] > idx[:, :-1][tie]).all(), "equal similarities not in index order"
    got_ref = torch.gather(ref_sim, 1, idx)
    got_bound = torch.gather(bound, 1, idx)
    assert ((sims - got_ref).abs() <= got_bound + 1e-30).all(), float(((sims - got_ref).abs() - got_bound).max())
    kth = torch.topk(ref_sim, k, dim=1).values[:, -1:]
    tol = 2 * bound.max(dim=1, keepdim=True).values
    surely_in = ref_sim > kth + tol      # must be returned
    maybe = (ref_sim - kth).abs() <= tol  # may or may not be returned
    returned = torch.zeros_like(ref_sim, dtype=torch.bool).scatter_(1, idx, True)
    assert (returned | ~surely_in).all(), "a clear top-k member is missing"
    assert (~returned | surely_in | maybe).all(), "a clear non-member was returned"
    assert returned.sum(1).eq(k).all(), "duplicate indices"


def vote_ref(sims, idx, labels, C, k, T):
    """fp64 weighted vote over the first k columns; NaN row and pred -1 for an out-of-range label."""
    s, i, lab = sims.double().cpu()[:, :k], idx.cpu()[:, :k], labels.cpu()
    Q = s.shape[0]
    scores = torch.zeros(Q, C, dtype=torch.float64)
    pred = torch.empty(Q, dtype=torch.int64)
    for q in range(Q):
        y = lab[i[q]]
        if ((y < 0) | (y >= C)).any():
            scores[q] = float("nan")
            pred[q] = -1
            continue
        scores[q].index_add_(0, y, torch.exp(s[q] / T))
        pred[q] = int(torch.argmax(scores[q]))  # torch.argmax returns the first maximal index
    return scores, pred


def pool_ref(feats: torch.Tensor, pool: str, normalize: str, with_cls: bool = True) -> torch.Tensor:
    """Pooling of (B, T, D) encoder outputs in fp64 (scripts/evaluation/visualize_representation.py:87-108)."""
    f = feats.double()
    if pool == "cls":
        out = f[:, 0]
    elif pool == "mean":
        out = f[:, 1:].mean(1) if with_cls else f.mean(1)
    else:
        out = f.mean(1)
    if normalize == "l2":
        out = out / (out.norm(dim=1, keepdim=True) + 1e-8)
    return out
