"""search_deep on the GPU, against the oracle of test_gpu_ivf.py built from the existing kernels
only -- transform(Q, X.float(), squared=True), the columns outside the probed lists masked, a
stable sort -- bit for bit, and the radix select's tables against their integer mirrors."""
import functools

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]


# ------------------------------------------------------------------------------- data
def _sizes(n, K):
    """Prescribed list sizes summing to n: an empty list, one row, a tile less one, a tile, a tile
    and one, two tiles and one, then the rest spread unevenly."""
    head = [0, 1, 15, 16, 17, 33][:K - 1]
    rest = K - len(head)
    left = n - sum(head)
    w = np.arange(1, rest + 1, dtype=np.float64)
    tail = np.floor(left * w / w.sum()).astype(np.int64)
    tail[-1] += left - tail.sum()
    return torch.tensor(head + tail.tolist(), dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _data(n, d, K, dtype, nq):
    """Rows around well-separated centres with prescribed list sizes, in shuffled order, and
    queries near rows (so every probe count meets populated lists)."""
    g = torch.Generator().manual_seed(n + 7 * K + d)
    C = 8.0 * torch.randn(K, d, generator=g)
    sizes = _sizes(n, K)
    lab = torch.repeat_interleave(torch.arange(K), sizes)[torch.randperm(n, generator=g)]
    X = (C[lab] + 0.25 * torch.randn(n, d, generator=g)).to(dtype)
    Q = (X[torch.randint(0, n, (nq,), generator=g)].float() + 0.25 * torch.randn(nq, d, generator=g)).to(dtype)
    return X.to(DEV), C.to(DEV), Q.to(DEV), sizes.to(DEV)


def _allowed(Q, X, C, nprobe):
    """bool [nq, n]: whether row i lies in one of query q's probed lists."""
    K, nq = C.shape[0], Q.shape[0]
    idx, d2 = ops.topk(X, C, 1)
    lab = torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1).long()
    probes = ops.topk(Q, C, nprobe)[0].long()
    member = torch.zeros((nq, K + 1), dtype=torch.bool, device=DEV)
    member.scatter_(1, probes, True)
    return member[:, torch.where(lab < 0, K, lab)]


def _oracle(Q, X, C, m, nprobe):
    """(rows, d2) from the existing kernels: the transform kernel's distances with the rows as
    centres, restricted to the probed lists, in a stable sort (equal values by row id)."""
    allowed = _allowed(Q, X, C, nprobe)
    Dm = ops.transform(Q, X.float(), squared=True)
    sv, si = torch.sort(torch.where(allowed, Dm, float("inf")), dim=1, stable=True)
    mm = min(m, X.shape[0])
    ok = torch.arange(m, device=DEV)[None, :] < allowed.sum(1)[:, None]
    rows = torch.full((Q.shape[0], m), -1, dtype=torch.int64, device=DEV)
    d2 = torch.full((Q.shape[0], m), float("nan"), device=DEV)
    rows[:, :mm], d2[:, :mm] = si[:, :mm], sv[:, :mm]
    return torch.where(ok, rows, -1), torch.where(ok, d2, float("nan"))


def _deep(index, Q, C, m, nprobe, **kw):
    return ops.index_decode(ops.index_search_deep(index, Q, C, m, nprobe, **kw))


def _assert_bitwise(got, exp):
    (rows, d2), (er, ed) = got, exp
    assert rows.dtype == torch.int64 and d2.dtype == torch.float32 and rows.shape == d2.shape == er.shape
    assert torch.equal(rows, er), int((rows != er).sum())
    assert torch.equal(d2.view(torch.int32), ed.view(torch.int32)), int((d2.view(torch.int32) != ed.view(torch.int32)).sum())


@functools.lru_cache(maxsize=None)
def _index(n, d, K, dtype, nq):
    X, C, _, _ = _data(n, d, K, dtype, nq)
    return ops.index_build(X, C)


BASE = (3000, 128, 37, 500)

# (n, D, K, nq, m, nprobe): just past the scan's list; recall@100; one probe, which pads; one query;
# the longest result over every list; odd widths and D = 300 and 1024; many short lists; a pair count
# past the launcher's small-batch rule, where the range passes run four pair blocks a wave (the
# histogram always one)
SEARCHES = [(*BASE, 33, 4), (*BASE, 100, 4), (*BASE, 100, 1), (3000, 128, 37, 1, 100, 4), (3000, 128, 37, 64, 2048, 37),
            (513, 30, 7, 17, 40, 3), (1200, 300, 20, 65, 64, 5), (700, 1024, 5, 33, 48, 2),
            (20011, 64, 1024, 300, 100, 16), (3000, 128, 37, 8200, 40, 16)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,m,nprobe", SEARCHES)
def test_search_deep_is_the_masked_sorted_transform_bitwise(native, dtype, n, d, K, nq, m, nprobe):
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    got = _deep(ix, Q, C, m, nprobe)
    _assert_bitwise(got, _oracle(Q, X, C, m, nprobe))
    again = _deep(ix, Q, C, m, nprobe)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [1, 8, 32])
def test_up_to_the_scan_length_it_is_search(native, dtype, m):
    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    for nprobe in (1, 4):
        assert torch.equal(ops.index_search_deep(ix, Q, C, m, nprobe), ops.index_search(ix, Q, C, m, nprobe))


@pytest.mark.parametrize("dtype", DTYPES)
def test_the_pass_count_and_the_blocking_do_not_change_the_keys(native, dtype):
    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    keys = ops.index_search_deep(ix, Q, C, 100, 4)
    for passes in (1, 2, 3, 4):
        assert torch.equal(ops.index_search_deep(ix, Q, C, 100, 4, passes=passes), keys), passes
    assert torch.equal(ops.index_search_deep(ix, Q, C, 100, 4, block_queries=77), keys)
    for passes in (0, 5):
        with pytest.raises(ValueError):
            ops.index_search_deep(ix, Q, C, 100, 4, passes=passes)
    for m in (0, 2049):
        with pytest.raises(ValueError):
            ops.index_search_deep(ix, Q, C, m, 4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,m,nprobe", [(*BASE, 100, 4), (*BASE, 33, 1), (513, 30, 7, 17, 40, 3),
                                               (3000, 128, 37, 8200, 40, 16)])
def test_tables_and_selects_equal_the_mirror(native, dtype, n, d, K, nq, m, nprobe):
    """Every pass's histogram and every select's (prefix, rank, hits, cand) as integers against
    ops.cpu.index_hist / index_select over the transform kernel's bits."""
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    probes = ops.topk(Q, C, nprobe)[0]
    member = _allowed(Q, X, C, nprobe)
    bits = ops.transform(Q, X.float(), squared=True).view(torch.int32).to(torch.int64)
    prefix = torch.zeros(nq, dtype=torch.int32, device=DEV)
    rank, hits, cand = (torch.zeros(nq, dtype=torch.int64, device=DEV) for _ in range(3))
    mp = mr = mc = None
    for p in range(4):
        table = ops.index_hist(ix, Q, probes, p, prefix)
        assert table.dtype == torch.int32 and table.shape == (nq, 256)
        assert torch.equal(ops.index_hist(ix, Q, probes, p, prefix, P=1), table)          # (and on every launch)
        exp = ref.index_hist(bits, member, mp, p)
        assert torch.equal(table.to(torch.int64) & 0xFFFFFFFF, exp), p
        twice = ops.index_hist(ix, Q, probes, p, prefix, table=table.clone())          # (only ever added into)
        assert torch.equal(twice.to(torch.int64), 2 * exp)
        ops.index_select(table, prefix, rank, hits, cand, m, p)
        mp, mr, mh, mc = ref.index_select(exp, mp, mr, mc, m, p)
        for got, want in ((prefix, mp), (rank, mr), (hits, mh), (cand, mc)):
            assert got.dtype == want.dtype and torch.equal(got, want), p
    assert torch.equal(cand, member.sum(1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_list_longer_than_a_flush_chunk(native, dtype):
    """A list of more than 65520 rows: the wave's 16-bit bins are flushed and zeroed on the way
    (csrc/deep.hip HIST_CHUNK), and pass 0 puts nearly all of the list on one bin (d2 is about
    2 D 0.25^2 = 4 with a deviation of 1, and [2, 8) is one top byte), more than 16 bits hold."""
    n, d, nq, m = 84000, 32, 5, 100
    g = torch.Generator().manual_seed(3)
    C = torch.stack([torch.zeros(d), torch.full((d,), 40.0)])
    lab = (torch.arange(n) >= 80500).long()
    X = (C[lab] + 0.25 * torch.randn(n, d, generator=g)).to(dtype).to(DEV)
    Q = (0.25 * torch.randn(nq, d, generator=g)).to(dtype).to(DEV)
    C = C.to(DEV)
    ix = ops.index_build(X, C)
    assert (ix.offsets[1:] - ix.offsets[:-1]).tolist() == [80500, 3500]
    probes = ops.topk(Q, C, 2)[0]
    bits = ops.transform(Q, X.float(), squared=True).view(torch.int32).to(torch.int64)
    member = torch.ones((nq, n), dtype=torch.bool, device=DEV)
    table = ops.index_hist(ix, Q, probes, 0)
    assert torch.equal(table.to(torch.int64), ref.index_hist(bits, member, None, 0)) and int(table.max()) > 65535
    prefix, _, _, _ = ref.index_select(table.to(torch.int64), None, None, None, m, 0)
    assert torch.equal(ops.index_hist(ix, Q, probes, 1, prefix).to(torch.int64), ref.index_hist(bits, member, prefix, 1))
    _assert_bitwise(_deep(ix, Q, C, m, 2), _oracle(Q, X, C, m, 2))


@pytest.mark.parametrize("dtype", DTYPES)
def test_exact_ties_go_to_the_lower_row(native, dtype):
    """Small integers (exact in bf16 and in the f32 accumulation) with rows i and i + n/2 identical:
    every row has a twin at the same distance, listed behind it, and where the m-th place is tied
    the radius lets more than m rows through, which does not disturb the first m."""
    n, d, K, nq, m = 1400, 24, 10, 300, 100
    g = torch.Generator().manual_seed(n + m)
    half = torch.randint(-3, 4, (n // 2, d), generator=g).float()
    X = torch.cat([half, half]).to(dtype).to(DEV)
    C = torch.randint(-3, 4, (K, d), generator=g).float().to(DEV)
    Q = torch.randint(-3, 4, (nq, d), generator=g).to(dtype).to(DEV)
    ix = ops.index_build(X, C)
    rows, d2 = _deep(ix, Q, C, m, K)
    _assert_bitwise((rows, d2), _oracle(Q, X, C, m, K))
    tie = d2[:, 1:] == d2[:, :-1]
    assert bool((rows[:, 1:][tie] > rows[:, :-1][tie]).all())
    assert float(tie.any(dim=1).float().mean()) >= 0.5
    # the exact radius (four passes) and its hits: more than m wherever the m-th distance is shared
    probes = ops.topk(Q, C, K)[0]
    prefix = torch.zeros(nq, dtype=torch.int32, device=DEV)
    rank, hits, cand = (torch.zeros(nq, dtype=torch.int64, device=DEV) for _ in range(3))
    for p in range(4):
        ops.index_select(ops.index_hist(ix, Q, probes, p, prefix), prefix, rank, hits, cand, m, p)
    assert torch.equal(prefix, d2[:, m - 1].view(torch.int32))
    Dm = ops.transform(Q, X.float(), squared=True)
    assert torch.equal(hits, (Dm <= d2[:, m - 1 : m]).sum(1)) and bool((hits > m).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_nan_query_leaves_the_others_unchanged(native, dtype):
    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    want = ops.index_search_deep(ix, Q, C, 100, 4)
    Qn = Q.clone()
    Qn[123, 5] = float("nan")
    got = ops.index_search_deep(ix, Qn, C, 100, 4)
    assert got.shape == want.shape
    keep = torch.arange(nq, device=DEV) != 123
    assert torch.equal(got[keep], want[keep])


def test_estimator_search_deep(native, monkeypatch):
    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, torch.bfloat16, nq)
    km = mikmeans.KMeans(K, dtype="bfloat16")
    km.cluster_centers_ = C
    ix = km.build_index(X)
    er, ed = _oracle(Q, X, C, 100, 4)
    rows, d2 = ix.search_deep(Q, 100, nprobe=4, squared=True)
    _assert_bitwise((rows, d2), (er, ed))
    rows, dist = ix.search_deep(Q, 100, nprobe=4)
    assert torch.equal(rows, er) and torch.equal(dist.view(torch.int32), ed.sqrt().view(torch.int32))
    # numpy queries in, numpy out, the host queries crossing in small blocks
    blocks = km._host_blocks
    monkeypatch.setattr(km, "_host_blocks", lambda Xh, block_rows=None: blocks(Xh, 97))
    nr, nd = ix.search_deep(Q.float().cpu().numpy(), 100, nprobe=4, squared=True, passes=3)
    assert isinstance(nr, np.ndarray) and isinstance(nd, np.ndarray) and nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nr, er.cpu().numpy()) and np.array_equal(nd, ed.cpu().numpy(), equal_nan=True)
    for bad in ((0, 4), (2049, 4), (40, 0), (40, K + 1)):
        with pytest.raises(ValueError):
            ix.search_deep(Q, bad[0], nprobe=bad[1])
    with pytest.raises(ValueError):
        ix.search(Q, 33, nprobe=4)
    none = km.build_index(X[:0])                                       # no rows: every slot empty
    er0, ed0 = none.search_deep(Q[:40], 50, nprobe=4)
    assert er0.shape == (40, 50) and bool((er0 == -1).all()) and bool(ed0.isnan().all())


def test_search_deep_refuses_what_does_not_fit(native, monkeypatch):
    from mikmeans.parallel import memplan

    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, torch.bfloat16, nq)
    km = mikmeans.KMeans(K, dtype="bfloat16")
    km.cluster_centers_ = C
    ix = km.build_index(X)
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", "100000")
    with pytest.raises(memplan.HBMCapacityError):
        ix.search_deep(Q, 100, nprobe=4)


def test_the_binding_refuses_wrong_tables(native):
    n, d, K, nq = BASE
    X, C, Q, _ = _data(n, d, K, torch.bfloat16, nq)
    ix = _index(n, d, K, torch.bfloat16, nq)
    probes = ops.topk(Q, C, 4)[0]
    prefix = torch.zeros(nq, dtype=torch.int32, device=DEV)
    i64 = torch.zeros(nq, dtype=torch.int64, device=DEV)
    table = torch.zeros((nq, 256), dtype=torch.int32, device=DEV)
    with pytest.raises(RuntimeError):
        ops.index_hist(ix, Q, probes, 0, table=table[:-1].contiguous())                 # a row short
    with pytest.raises(RuntimeError):
        ops.index_hist(ix, Q, probes, 0, table=table.to(torch.int64))
    with pytest.raises(RuntimeError):
        ops.index_hist(ix, Q, probes, 1, None)                                          # passes 1..3 take a prefix
    with pytest.raises(RuntimeError):
        ops.index_hist(ix, Q, probes, 4, prefix)
    with pytest.raises(RuntimeError):
        ops.index_hist(ix, Q, probes, 0, P=2)
    with pytest.raises(RuntimeError):
        native.ivf_select(table, prefix, i64, i64, i64, 2049, 0)
    with pytest.raises(RuntimeError):
        native.ivf_select(table, prefix[:-1].contiguous(), i64, i64, i64, 5, 0)
    with pytest.raises(RuntimeError):
        native.ivf_select(table, prefix, i64, i64, i64, 5, 4)
    assert native.IVF_DEEP_MAX_M == ops.INDEX_DEEP_MAX_M == 2048
    assert native.ivf_hist_blocks(1, 128, 100) == 1 and native.ivf_hist_blocks(1, 128, 1 << 20) == 1
