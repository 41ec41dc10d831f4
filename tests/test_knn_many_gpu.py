"""The many-query flat scan + top-k (knn.hip knn_topk_many_kernel, nq > 16 through K.knn_topk) against
torch.topk of fp32 scores, at the edges of its plan: ragged query groups and tiles, spans that end off
a row group, fewer rows than k, and data that passes (or ties) every running threshold."""
import pytest
import torch

from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.ops import reference as R
from copilot_for_consensus_amd.ops import _native

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _plan(nq, k, dim, rows):
    """(query tile, span rows, candidate slots, spans) the kernel uses for this problem."""
    out = torch.empty(4, dtype=torch.int32)
    _native.check(_native.kernels().cfc_knn_many_plan(nq, k, dim, rows, out.data_ptr()), "cfc_knn_many_plan")
    return out.tolist()


def _shape(nq, spans, k, dim):
    """nq: an int, or 'tile' / 'tile+2' of the plan for 128 queries; rows = spans * span + 37."""
    qt = _plan(128, k, dim, 1)[0]
    nq = {"tile": qt, "tile+2": qt + 2}.get(nq, nq)
    span = _plan(nq, k, dim, 1)[1]
    rows = spans * span + 37
    assert _plan(nq, k, dim, rows)[1] == span     # small problems sit at the span's lower bound
    return nq, rows


# nq, spans (rows = spans * span + 37; 0: fewer rows than k), k, dim, metric, dead share, row_lo
CASES = [(17, 2, 10, 384, "dot", 0.1, 13), ("tile", 2, 10, 384, "l2", 0.1, 13), ("tile+2", 2, 10, 384, "dot", 0.1, 0),
         ("tile+2", 2, 150, 384, "l2", 0.1, 5), ("tile", 1, 256, 384, "dot", 0.0, 13), (17, 2, 1, 128, "l2", 0.1, 7),
         ("tile+2", 2, 10, 128, "dot", 0.0, 13), (17, 1, 256, 1024, "dot", 0.1, 3), ("tile+2", 2, 10, 1024, "l2", 0.1, 13),
         ("tile", 1, 150, 1024, "dot", 0.0, 0), (40, 0, 150, 384, "dot", 0.0, 3), (33, 0, 256, 128, "l2", 0.0, 0)]


@pytest.mark.parametrize("nq,spans,k,dim,metric,dead,lo", CASES)
def test_knn_topk_many_matches_reference(nq, spans, k, dim, metric, dead, lo):
    torch.manual_seed(0)
    nq, rows = _shape(nq, spans, k, dim)
    N = lo + rows
    X = torch.nn.functional.normalize(torch.randn(N, dim, device=DEV), dim=1).bfloat16()
    Q = torch.nn.functional.normalize(torch.randn(nq, dim, device=DEV), dim=1).bfloat16()
    alive = torch.rand(N, device=DEV) >= dead
    xn2 = X.float().pow(2).sum(1) if metric == "l2" else None
    qn2 = Q.float().pow(2).sum(1) if metric == "l2" else None
    v, i = K.knn_topk(X, Q, k, xn2, qn2, alive if dead else None, row_lo=lo, N=N)
    ref = R.knn_scores(X[lo:].float(), Q.float(), None if xn2 is None else xn2[lo:], qn2)
    ref = ref.masked_fill(~alive[lo:][None], float("-inf"))
    rv, ri = torch.topk(ref, min(k, N - lo), dim=1)
    assert v.shape == rv.shape
    assert torch.allclose(v, rv, atol=2e-3, rtol=1e-3), (v[:, :5], rv[:, :5])
    # the returned rows really have those scores
    got = torch.gather(ref, 1, (i - lo).clamp_min(0))
    assert torch.allclose(got, v, atol=2e-3, rtol=1e-3)
    assert bool((i >= lo).all()) and bool((i < N).all()) and bool(alive[i].all())
    s = i.sort(1).values
    assert bool((s[:, 1:] != s[:, :-1]).all())           # no row twice for one query


@pytest.mark.parametrize("k", [10, 256])
@pytest.mark.parametrize("order", ["ascending", "descending", "identical"])
def test_knn_topk_many_exact_when_the_threshold_never_helps(order, k):
    """X_i = a_i e_0, Q_j = 2^(j % 4) e_0 with bf16-exact a_i: every score is exact in fp32 and ordered
    the same way for every query.  Ascending: every row passes every threshold (the buffers fill and
    are cut all the way); descending: nothing passes after the first k; identical: every score ties."""
    nq, N = _shape("tile+2", 2, k, 384)
    # consecutive positive bf16 bit patterns from 2^-64 up: strictly ascending, 8-bit significands
    a = ((63 << 7) + torch.arange(N, device=DEV)).to(torch.int16).view(torch.bfloat16).float()
    a = {"ascending": a, "descending": a.flip(0), "identical": torch.full_like(a, 3.0)}[order]
    assert bool((a.bfloat16().float() == a).all())
    X = torch.zeros(N, 384, device=DEV, dtype=torch.bfloat16)
    X[:, 0] = a.bfloat16()
    Q = torch.zeros(nq, 384, device=DEV, dtype=torch.bfloat16)
    Q[:, 0] = (2.0 ** (torch.arange(nq, device=DEV) % 4)).bfloat16()
    v, i = K.knn_topk(X, Q, k)
    ref = Q[:, :1].float() * X[:, 0].float()[None, :]        # the one non-zero term of each dot product
    assert torch.equal(v, torch.topk(ref, k, dim=1).values)
    assert torch.equal(torch.gather(ref, 1, i), v)
    s = i.sort(1).values
    assert bool((s[:, 1:] != s[:, :-1]).all()) and bool((i >= 0).all()) and bool((i < N).all())


def test_query_batch_of_40_matches_single_queries():
    from copilot_for_consensus_amd.vectorstore import HipFlatIndex
    g = torch.Generator(device=DEV).manual_seed(3)
    C = torch.nn.functional.normalize(torch.randn(40, 384, device=DEV, generator=g), dim=1)
    X = C[torch.randint(0, 40, (5000,), device=DEV, generator=g)] + 0.05 * torch.randn(5000, 384, device=DEV, generator=g)
    flat = HipFlatIndex(384, device=DEV, capacity=1 << 13)
    flat.add_embeddings([f"v{j}" for j in range(5000)], X)
    Q = C + 0.05 * torch.randn(40, 384, device=DEV, generator=g)
    for deleted in (False, True):
        if deleted:
            for j in range(0, 5000, 7):
                flat.delete(f"v{j}")
        batch = [[r.id for r in row] for row in flat.query_batch(Q, top_k=10)]
        single = [[r.id for r in flat.query(q, top_k=10)] for q in Q]
        assert batch == single
        assert all(len(row) == 10 for row in batch)
