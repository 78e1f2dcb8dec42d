"""The refined PQ search on the GPU: the re-rank kernel of csrc/rerank.hip against an oracle of
separate torch.sub / mul / add on the device in the canonical order, the shortlist against the group
rule over the oracle of tests/test_gpu_pq.py, and the whole search -- against the oracle, from run to
run, across the query blocking, with host rows, and exactly on integer data.  Every comparison is
bitwise."""
import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops

from .test_gpu_pq import COPIES, K, LONG, NQ, SIZES, Case, _cases, _name

pytestmark = pytest.mark.gpu

EMPTY = ops.IVF_EMPTY_KEY
DEV = "cuda:0"


def oracle_keys(Q, X, cand):
    """[nq, R] keys by the definition: float32 operands, pieces of V columns, accumulator s of sixteen
    takes the pieces s, s + 16, ... column after column by torch.sub, torch.mul, torch.add (one
    rounding each), the accumulators meet as ((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7)) and the same over
    a8..a15; every NaN is 0x7fc00000; an id outside [0, n) is EMPTY."""
    nq, F = Q.shape
    n, R = X.shape[0], cand.shape[1]
    V = 8 if Q.dtype == torch.bfloat16 else 4
    rounds = ((F + V - 1) // V + 15) // 16
    ok = (cand >= 0) & (cand < n)
    c = torch.where(ok, cand, 0)
    d = torch.sub(Q.to(torch.float32)[:, None, :], X.to(torch.float32)[c.reshape(-1)].view(nq, R, F))
    p = torch.zeros((nq, R, rounds * 16 * V), dtype=torch.float32, device=Q.device)
    p[:, :, :F] = torch.mul(d, d)
    p = p.view(nq, R, rounds, 16, V)
    a = torch.zeros((nq, R, 16), dtype=torch.float32, device=Q.device)
    for k in range(rounds):
        for e in range(V):
            a = torch.add(a, p[:, :, k, :, e])
    a = a.unbind(-1)

    def half(o):
        return torch.add(torch.add(torch.add(a[o], a[o + 1]), torch.add(a[o + 2], a[o + 3])),
                         torch.add(torch.add(a[o + 4], a[o + 5]), torch.add(a[o + 6], a[o + 7])))

    d2 = torch.add(half(0), half(8))
    bits = torch.where(torch.isnan(d2), 0x7FC00000, torch.nan_to_num(d2, nan=0.0, posinf=float("inf")).contiguous()
                       .view(torch.int32).to(torch.int64))
    return torch.where(ok, (bits << 32) | c, EMPTY)


def top(keys, m):
    out = torch.full((keys.shape[0], m), EMPTY, dtype=torch.int64, device=keys.device)
    k = keys.sort(dim=1).values[:, :m]
    out[:, : k.shape[1]] = k
    return out


N_ROWS = 300
NAN_ROW, INF_ROW = 17, 230


def _rows(F, dtype, seed=0):
    g = torch.Generator().manual_seed(1000 * F + seed)
    X = (torch.randn(N_ROWS, F, generator=g) * 2).to(dtype)
    X[NAN_ROW, F // 2] = float("nan")
    X[INF_ROW, F - 1] = float("inf")
    Q = (torch.randn(5, F, generator=g) * 2).to(dtype)
    return X.to(DEV), Q.to(DEV), g


def _cands(g, nq, R):
    cand = torch.randint(0, N_ROWS, (nq, R), generator=g)
    spots = torch.randperm(R, generator=g)
    for at, v in zip(spots.tolist(), (NAN_ROW, INF_ROW, -1, N_ROWS, N_ROWS + 7, 2 ** 40, -(2 ** 33))):
        cand[:, at] = v                                   # (R = 1, 3, 4, 5 take the first few of these)
    if R >= 3:
        cand[:, spots[0]] = cand[:, (spots[0] + 1) % R]   # a duplicate
    return cand.to(DEV)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
@pytest.mark.parametrize("F", [8, 20, 24, 136, 1024])
def test_rerank_against_the_device_oracle(F, dtype):
    X, Q, g = _rows(F, dtype)
    for nq in (1, 5):
        for R in (1, 3, 4, 5, 64, 65, 257):
            cand = _cands(g, nq, R)
            want = oracle_keys(Q[:nq], X, cand)
            got = ops.rerank(Q[:nq], X, cand, R)
            assert got.dtype == torch.int64 and got.shape == (nq, R)
            assert torch.equal(got, top(want, R)), (nq, R)
            assert torch.equal(ops.rerank(Q[:nq], X, cand, min(R, 10)), top(want, min(R, 10))), (nq, R)
            assert torch.equal(ops.rerank(Q[:nq], X, cand, R + 3), top(want, R + 3)), (nq, R)
    # and the mirror on the host gives the same bits
    cand = _cands(g, 5, 65)
    assert torch.equal(ops.rerank(Q, X, cand, 65).cpu(), ops.rerank(Q.cpu(), X.cpu(), cand.cpu(), 65))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
def test_non_finite_rows_sort_behind_the_finite_and_before_the_padding(dtype):
    X, Q, g = _rows(24, dtype)
    cand = torch.tensor([[NAN_ROW, 5, -1, INF_ROW, 9, N_ROWS, 5]], device=DEV).expand(5, 7).contiguous()
    keys = ops.rerank(Q, X, cand, 7)
    rows, d2 = ops.index_decode(keys)
    assert rows[:, 3:].tolist() == [[INF_ROW, NAN_ROW, -1, -1]] * 5
    assert bool(torch.isfinite(d2[:, :3]).all()) and sorted(rows[0, :3].tolist()) == [5, 5, 9]
    assert bool(torch.isinf(d2[:, 3]).all()) and bool((keys[:, 4] >> 32 == 0x7FC00000).all())
    assert bool((d2[:, :3] >= 0).all()) and bool((d2[:, 1:3] >= d2[:, 0:2]).all())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
@pytest.mark.parametrize("F", [20, 24, 136])
def test_rows_as_a_column_slice_of_a_wider_tensor(F, dtype):
    X, Q, g = _rows(F, dtype, seed=1)
    cand = _cands(g, 5, 65)
    want = top(oracle_keys(Q, X, cand), 65)
    V = 8 if dtype == torch.bfloat16 else 4
    for width, col in ((F + 3 * V, V), (F + 3 * V, 3), (F + 2 * V + 1, 0), (F + 2 * V + 1, V)):
        W = torch.randn(N_ROWS, width, device=DEV).to(dtype)        # aligned or not: the pointer, the stride
        W[:, col : col + F] = X
        Xs = W[:, col : col + F]
        assert Xs.stride(0) == width and not Xs.is_contiguous()
        assert torch.equal(ops.rerank(Q, Xs, cand, 65), want), (width, col)
    Wq = torch.randn(5, F + 5, device=DEV).to(dtype)
    Wq[:, 1 : 1 + F] = Q
    assert torch.equal(ops.rerank(Wq[:, 1 : 1 + F], X, cand, 65), want)
    assert torch.equal(ops.rerank(Q[2:3], X[:1], torch.zeros((1, 2), dtype=torch.int64, device=DEV), 2),
                       top(oracle_keys(Q[2:3], X[:1], torch.zeros((1, 2), dtype=torch.int64, device=DEV)), 2))


# ---------------------------------------------------------------- the shortlist and the whole search
@pytest.fixture(params=[torch.bfloat16, torch.float32], ids=_name)
def case(request):
    key = (64, 16, request.param)
    if key not in _cases:
        _cases[key] = Case(*key)
    return _cases[key]


def shortlist_oracle(case, S, nprobe):
    """[NQ, nprobe * S] row ids by the group rule, from the ADC bits of the scan's oracle: position p of
    a list is in group (p // 256) mod G and a group keeps its s smallest (bits, row)."""
    G, s = (1, S) if S <= 32 else (S // 32, 32)
    keys, probes = case.oracle(nprobe)                                       # sorted keys over all rows
    n, dev = case.n, case.dev
    val = keys.clone()
    rows = torch.where(keys == EMPTY, n, keys & 0xFFFFFFFF)
    by_row = torch.full((NQ, n + 1), EMPTY, dtype=torch.int64, device=dev)   # (slot n: the rows not probed)
    by_row.scatter_(1, rows, val)
    by_row = by_row[:, :n]
    ix = case.index
    pos = torch.empty(n, dtype=torch.int64, device=dev)
    pos[ix.order] = torch.arange(n, device=dev) - ix.offsets[case.lab[ix.order]]
    grp = (pos // 256) % G
    assert G == 1 or int(grp[case.lab == LONG].max()) == G - 1               # the 2100-row list fills every group
    out = torch.full((NQ, nprobe, G, s), -1, dtype=torch.int64, device=dev)
    for j in range(nprobe):
        for g_ in range(G):
            mine = (case.lab[None, :] == probes[:, j : j + 1]) & (grp[None, :] == g_)
            k = torch.where(mine, by_row, EMPTY).sort(dim=1).values[:, :s]
            out[:, j, g_, :] = torch.where(k == EMPTY, -1, k & 0xFFFFFFFF)
    return out.view(NQ, nprobe * S)


@pytest.mark.parametrize("S", [5, 32, 256])
def test_shortlist_against_the_oracle(case, S):
    for nprobe in (3, K):
        want = shortlist_oracle(case, S, nprobe)
        got = ops.pq_shortlist(case.index, case.Q, case.C, S, nprobe)
        assert got.dtype == torch.int64 and torch.equal(got, want), (S, nprobe)
        for block in (1, 7):
            assert torch.equal(ops.pq_shortlist(case.index, case.Q, case.C, S, nprobe, block_queries=block), want)
    # the copies' query: its nearest list is the long one, and the 41 equal rows come in row order
    got = ops.pq_shortlist(case.index, case.Q[:1], case.C, S, 1).view(-1)
    assert int((got >= 0).sum()) == S
    if S == 32:
        assert torch.equal(got, case.copy_ids[:32])


@pytest.mark.parametrize("S,nprobe,m", [(5, 3, 10), (32, 3, 10), (256, K, 32), (64, 1, 32)])
def test_refined_search_end_to_end(case, S, nprobe, m):
    F = case.F
    cand = shortlist_oracle(case, S, nprobe)
    want = top(oracle_keys(case.Q[:, :F], case.X, cand), m)
    keys = ops.pq_refine(case.index, case.Q, case.C, case.X, m, nprobe, S)
    assert torch.equal(keys, want)
    assert torch.equal(ops.pq_refine(case.index, case.Q, case.C, case.X, m, nprobe, S), keys)         # run to run
    for block in (1, NQ):
        assert torch.equal(ops.pq_refine(case.index, case.Q, case.C, case.X, m, nprobe, S, block_queries=block), keys)
    Xh = case.X.cpu()
    assert torch.equal(ops.pq_refine(case.index, case.Q, case.C, Xh, m, nprobe, S), keys)             # host rows
    assert torch.equal(ops.pq_refine(case.index, case.Q, case.C, Xh, m, nprobe, S, block_queries=5), keys)
    # the public interface
    km = mikmeans.KMeans(K, dtype=_name(case.dtype), device=case.dev)
    km.cluster_centers_ = case.C.clone()
    ix = mikmeans.PQIndex(km, case.index)
    r0, d0 = ops.index_decode(want)
    rows, d2 = ix.search(case.Q, m, nprobe=nprobe, squared=True, refine=case.X, shortlist=S)
    assert torch.equal(rows, r0) and torch.equal(d2.view(torch.int32), d0.view(torch.int32))
    rows, d = ix.search(case.Q, m, nprobe=nprobe, refine=Xh, shortlist=S)
    assert torch.equal(rows, r0) and torch.equal(d.view(torch.int32), d0.sqrt().view(torch.int32))
    rn, dn = ix.search(case.Q.float().cpu().numpy(), m, nprobe=nprobe, refine=Xh.float().numpy(), shortlist=S)
    assert np.array_equal(rn, r0.cpu().numpy()) and np.array_equal(dn.view(np.int32), d.cpu().numpy().view(np.int32))
    if nprobe == 1:                                                          # padding: the 0-, 1- and 15-row lists
        assert (rows[NQ - 3 :] >= 0).sum(1).tolist() == [0, 1, 15]
        assert bool(((rows == -1) == torch.isnan(d)).all())


def test_refined_search_errors(case):
    km = mikmeans.KMeans(K, dtype=_name(case.dtype), device=case.dev)
    km.cluster_centers_ = case.C.clone()
    ix = mikmeans.PQIndex(km, case.index)
    other = torch.float32 if case.dtype == torch.bfloat16 else torch.bfloat16
    with pytest.raises(ValueError, match="read in place"):
        ix.search(case.Q, 3, refine=case.X.to(other))
    with pytest.raises(ValueError, match="only with refine"):
        ix.search(case.Q, 3, shortlist=32)
    with pytest.raises(ValueError, match="shortlist"):
        ix.search(case.Q, 3, refine=case.X, shortlist=48)
    with pytest.raises(ValueError, match="refine takes the rows"):
        ix.search(case.Q, 3, refine=case.X[:-1])
    # search without refine is what it was
    r0, d0 = ops.index_decode(ops.pq_search(case.index, case.Q, case.C, 10, 3))
    rows, d2 = ix.search(case.Q, 10, nprobe=3, squared=True)
    assert torch.equal(rows, r0) and torch.equal(d2.view(torch.int32), d0.view(torch.int32))


def test_integer_data_full_probe_is_the_exact_search():
    """Coordinates in [-8, 8]: every subtract, multiply and add is exact, so with every list probed and
    no list longer than the shortlist the refined search is the brute-force m-nearest by (distance, row),
    and for s >= m it keeps every true neighbour the codes alone found."""
    g = torch.Generator().manual_seed(7)
    X = torch.randint(-8, 9, (640, 24), generator=g).to(torch.float32)
    Q = torch.randint(-8, 9, (48, 24), generator=torch.Generator().manual_seed(8)).to(torch.float32)
    d = ((Q.double()[:, None, :] - X.double()[None, :, :]) ** 2).sum(-1)
    order = torch.argsort(d, dim=1, stable=True)
    km = mikmeans.KMeans(64, dtype="float32", device=DEV, seed=1)
    km.cluster_centers_ = X[:64].clone().to(DEV)
    Xd, Qd = X.to(DEV), Q.to(DEV)
    ix = km.build_pq_index(Xd, 8, train_rows=640, pq_max_iter=2)
    assert int(ix.list_sizes.max()) <= 32
    for m in (1, 10, 32):
        for rows_at in (Xd, X):
            rows, d2 = ix.search(Qd, m, nprobe=64, squared=True, refine=rows_at, shortlist=32)
            assert torch.equal(rows.cpu(), order[:, :m])
            assert torch.equal(d2.cpu().double(), d.gather(1, order[:, :m]))
    for nprobe, S, m in ((4, 10, 10), (8, 64, 32), (16, 1, 1)):
        plain, _ = ix.search(Qd, m, nprobe=nprobe)
        fine, _ = ix.search(Qd, m, nprobe=nprobe, refine=Xd, shortlist=S)
        for q in range(Q.shape[0]):
            held = set(order[q, :m].tolist()) & set(plain[q].tolist())
            assert held <= set(fine[q].tolist()), (nprobe, S, m, q)
