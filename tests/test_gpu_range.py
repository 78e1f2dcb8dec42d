"""range_search / range_count on the GPU (csrc/range.hip), bit for bit against an oracle built from
the existing kernels only -- transform(Q, X.float(), squared=True), the columns outside the probed
lists masked out, the values <= r2[q] kept, a stable sort over (value, row id).  (The CPU mirror:
test_range.py.)"""
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


@functools.lru_cache(maxsize=None)
def _index(n, d, K, dtype, nq):
    X, C, _, _ = _data(n, d, K, dtype, nq)
    return ops.index_build(X, C)


def _lists(X, C):
    idx, d2 = ops.topk(X, C, 1)
    return torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1).long()


def _radii(nq, d):
    """r2[q] = D (0, 0.08, 0.1875, 0.25, 1e6)[q % 5]: no hit, about the one source row, about half
    of its cluster, most of its cluster, everything probed."""
    f = torch.tensor([0.0, 0.08, 0.1875, 0.25, 1e6], dtype=torch.float64) * d
    return f[torch.arange(nq) % 5].float().to(DEV)


class _Oracle:
    """From the existing kernels: the transform kernel's distances with the rows as centres,
    restricted to the probed lists and to d2 <= r2[q]; per query in a stable sort (equal values by
    row id), or probe after probe and ascending row within a probe."""

    def __init__(self, Q, X, C, r2, nprobe):
        K, nq, n = C.shape[0], Q.shape[0], X.shape[0]
        lab = _lists(X, C)
        lab = torch.where(lab < 0, K, lab)
        probes = ops.topk(Q, C, nprobe)[0].long()
        prank = torch.full((nq, K + 1), nprobe, dtype=torch.int64, device=DEV)
        prank.scatter_(1, probes, torch.arange(nprobe, device=DEV).expand(nq, -1))
        Dm = ops.transform(Q, X.float(), squared=True)
        self.hit = hit = (prank[:, lab] < nprobe) & (Dm <= r2[:, None])
        self.counts = hit.sum(1)
        self.lims = torch.zeros(nq + 1, dtype=torch.int64, device=DEV)
        self.lims[1:] = torch.cumsum(self.counts, 0)
        sv, si = torch.sort(torch.where(hit, Dm, float("inf")), dim=1, stable=True)
        ok = torch.arange(n, device=DEV)[None, :] < self.counts[:, None]
        self.rows, self.d2 = si[ok], sv[ok]
        q, i = hit.nonzero(as_tuple=True)                           # query-major, ascending row
        o = torch.argsort(q * nprobe + prank[q, lab[i]], stable=True)
        self.urows, self.ud2 = i[o], Dm[q, i][o]
        # hits per (query, list), and every list's size
        onehot = torch.zeros((n, K + 1), dtype=torch.float32, device=DEV)
        onehot[torch.arange(n, device=DEV), lab] = 1.0
        self.per_list = (hit.float() @ onehot)[:, :K].long()
        self.sizes = onehot.sum(0)[:K].long()


def _bits(t):
    return t.view(torch.int32)


def _range(index, Q, C, r2, nprobe, **kw):
    lims, keys = ops.index_range(index, Q, C, r2, nprobe, **kw)
    rows, d2 = ops.index_decode(keys)
    assert lims.dtype == rows.dtype == torch.int64 and d2.dtype == torch.float32
    return lims, rows, d2


def _assert_bitwise(got, lims, rows, d2):
    assert got[0].shape == lims.shape and torch.equal(got[0], lims), int((got[0] != lims).sum())
    assert got[1].shape == rows.shape and torch.equal(got[1], rows), int((got[1] != rows).sum())
    assert torch.equal(_bits(got[2]), _bits(d2)), int((_bits(got[2]) != _bits(d2)).sum())


# (n, D, K, nq, nprobe): the base shape, one probe and every list (the exact search); D -> DPAD 32;
# ragged wide rows; DPAD 1024; many short lists (whole lists inside one tile); one query; a pair
# count past the launcher's small-batch rule (32768 P pairs, P = 4 at D = 128), which runs four
# pair blocks a wave
RANGES = [(3000, 128, 37, 500, 4), (3000, 128, 37, 500, 1), (3000, 128, 37, 500, 37), (513, 30, 7, 17, 3),
          (1200, 300, 20, 65, 5), (700, 1024, 5, 33, 2), (20011, 64, 1024, 300, 16), (3000, 128, 37, 1, 4),
          (3000, 128, 37, 8200, 16)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,nprobe", RANGES)
def test_range_is_the_masked_thresholded_transform_bitwise(native, dtype, n, d, K, nq, nprobe):
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    r2 = _radii(nq, d)
    o = _Oracle(Q, X, C, r2, nprobe)
    # what keeps the test honest, on the oracle.  (One query is query 0, whose radius is 0: it is the
    # query without a hit, and the share of queries with one is asked of the other shapes.)
    assert bool((o.counts == 0).any())
    if nq > 1:
        assert float((o.counts > 0).float().mean()) >= 0.6
        assert int(o.per_list.max()) > 16
        assert bool(((o.per_list > 0) & (o.per_list < o.sizes[None, :])).any())
        if nprobe > 1:
            assert bool(((o.per_list > 0).sum(1) >= 2).any())
    if nq == 8200:
        assert native.ivf_range_blocks(1 if dtype == torch.bfloat16 else 0, ix.cols, nq * nprobe) > 1
    got = _range(ix, Q, C, r2, nprobe)
    _assert_bitwise(got, o.lims, o.rows, o.d2)
    again = _range(ix, Q, C, r2, nprobe)
    _assert_bitwise(again, *got)
    uns = _range(ix, Q, C, r2, nprobe, sort=False)
    _assert_bitwise(uns, o.lims, o.urows, o.ud2)
    _assert_bitwise(_range(ix, Q, C, r2, nprobe, sort=False), *uns)
    assert torch.equal(ops.index_range(ix, Q, C, r2, nprobe, count_only=True), o.counts)
    if nq == 1:                                                     # the one query with everything probed
        big = torch.full((1,), 1e6 * d, device=DEV)
        ob = _Oracle(Q, X, C, big, nprobe)
        assert int(ob.counts[0]) > 16
        _assert_bitwise(_range(ix, Q, C, big, nprobe), ob.lims, ob.rows, ob.d2)
        _assert_bitwise(_range(ix, Q, C, big, nprobe, sort=False), ob.lims, ob.urows, ob.ud2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_lists_probed_by_few_and_many_queries(native, dtype):
    """One probe per query, the queries placed on chosen centres: lists probed by 1, 16, 17 and 70
    queries (one pair, a full block, a block and one, five blocks) and a list nobody probes; under
    a radius that takes everything, every query gets its probed list, nearest row first."""
    n, d, K = 3000, 128, 37
    X, C, _, sizes = _data(n, d, K, dtype, 64)
    ix = _index(n, d, K, dtype, 64)
    want = {6: 1, 9: 16, 12: 17, 20: 70}
    g = torch.Generator().manual_seed(5)
    Q = torch.cat([C[k].cpu() + 0.25 * torch.randn(c, d, generator=g) for k, c in want.items()])
    Q = Q[torch.randperm(Q.shape[0], generator=g)].to(dtype).to(DEV)
    probe = ops.topk(Q, C, 1)[0][:, 0].long()
    probed = torch.bincount(probe, minlength=K)
    assert {k: int(probed[k]) for k in want} == want and int(probed.sum()) == sum(want.values())
    r2 = torch.full((Q.shape[0],), 1e6 * d, device=DEV)
    o = _Oracle(Q, X, C, r2, 1)
    lims, rows, d2 = _range(ix, Q, C, r2, 1)
    _assert_bitwise((lims, rows, d2), o.lims, o.rows, o.d2)
    assert torch.equal(lims[1:] - lims[:-1], sizes[probe])
    km = mikmeans.KMeans(K, dtype=str(dtype).replace("torch.", ""))
    km.cluster_centers_ = C
    cix = km.build_index(X)
    Dm = ops.transform(Q, X.float(), squared=True)
    for q in range(Q.shape[0]):
        mine = cix.rows_of(int(probe[q]))
        exp = mine[torch.sort(Dm[q, mine], stable=True).indices]
        assert torch.equal(rows[lims[q] : lims[q + 1]], exp), q
    _assert_bitwise(_range(ix, Q, C, r2, 1, sort=False), o.lims, o.urows, o.ud2)


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_agrees_with_search(native, dtype):
    """r2[q] = the m-th squared distance of search: the first m hits are search's rows and bits,
    and every later hit lies at exactly that distance."""
    n, d, K, nq, m, nprobe = 3000, 128, 37, 500, 8, 4
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    srows, sd2 = ops.index_decode(ops.index_search(ix, Q, C, m, nprobe))
    full = srows[:, m - 1] >= 0                                      # the probed lists hold at least m rows
    assert float(full.float().mean()) >= 0.9
    Qf, srows, sd2 = Q[full], srows[full], sd2[full]
    lims, rows, d2 = _range(ix, Qf, C, sd2[:, m - 1].contiguous(), nprobe)
    counts = lims[1:] - lims[:-1]
    assert bool((counts >= m).all())
    first = lims[:-1, None] + torch.arange(m, device=DEV)[None, :]
    assert torch.equal(rows[first], srows) and torch.equal(_bits(d2[first]), _bits(sd2))
    qid = torch.repeat_interleave(torch.arange(Qf.shape[0], device=DEV), counts)
    assert torch.equal(_bits(d2), _bits(torch.minimum(d2, sd2[qid, m - 1])))     # none beyond the radius
    later = torch.arange(rows.numel(), device=DEV) >= lims[qid] + m
    assert torch.equal(_bits(d2[later]), _bits(sd2[qid, m - 1][later]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq", [(1400, 24, 10, 300), (600, 300, 6, 70)])
def test_range_exact_ties(native, dtype, n, d, K, nq):
    """Small integers (exact in bf16 and in the f32 accumulation) with rows i and i + n/2 identical,
    every list probed and integer radii: the hits are the float64 brute force's exactly, equal
    distances go to the lower row -- a row's twin is a hit with it and behind it, directly behind
    it wherever no third row lies at that distance -- and r2 = 0 returns exactly the rows identical
    to the query."""
    g = torch.Generator().manual_seed(n + 8)
    half = torch.randint(-3, 4, (n // 2, d), generator=g).float()
    X = torch.cat([half, half]).to(dtype).to(DEV)
    C = torch.randint(-3, 4, (K, d), generator=g).float().to(DEV)
    Q = torch.randint(-3, 4, (nq, d), generator=g).to(dtype).to(DEV)
    Q[: nq // 4] = X[: nq // 4]                                      # queries that are rows: a hit at 0
    ix = ops.index_build(X, C)
    Qd, Xd = Q.double(), X.double()                                  # (integers: every f64 operation is exact)
    exact = (Qd * Qd).sum(1)[:, None] + (Xd * Xd).sum(1)[None, :] - 2 * (Qd @ Xd.T)
    near = exact.sort(dim=1).values
    # r2 by query class: 0, the 2nd, the 9th and the 40th smallest distance of the query
    r2 = torch.stack([torch.zeros(nq, dtype=torch.float64, device=DEV), near[:, 1], near[:, 8], near[:, 39]], 1)
    r2 = r2[torch.arange(nq, device=DEV), torch.arange(nq, device=DEV) % 4].float()
    hit = exact <= r2[:, None].double()
    sv, si = torch.sort(torch.where(hit, exact, float("inf")), dim=1, stable=True)
    counts = hit.sum(1)
    ok = torch.arange(n, device=DEV)[None, :] < counts[:, None]
    lims, rows, d2 = _range(ix, Q, C, r2, K)
    assert torch.equal(lims[1:] - lims[:-1], counts) and torch.equal(rows, si[ok]) and torch.equal(d2.double(), sv[ok])
    assert bool((counts % 2 == 0).all()) and int(counts.max()) >= 40 and int((counts == 0).sum()) > 0
    qid = torch.repeat_interleave(torch.arange(nq, device=DEV), counts)
    tie = (d2[1:] == d2[:-1]) & (qid[1:] == qid[:-1])
    assert bool((rows[1:] > rows[:-1])[tie].all())
    lower = (rows < n // 2).nonzero().flatten()
    nxt = (lower + 1).clamp_max(rows.numel() - 1)
    adjacent = (rows[nxt] == rows[lower] + n // 2) & (qid[nxt] == qid[lower])
    # (within equal distances the lower twins come first, so those of one distance follow each other)
    shared = (d2[lower][1:] == d2[lower][:-1]) & (qid[lower][1:] == qid[lower][:-1])
    lone = torch.ones_like(adjacent)                                 # lower twins whose distance only the twin shares
    lone[1:] &= ~shared
    lone[:-1] &= ~shared
    assert int(lone.sum()) > nq // 8 and bool(adjacent[lone].all())
    zero = (torch.arange(nq, device=DEV) % 4 == 0)
    for q in zero.nonzero().flatten().tolist():
        same = (X == Q[q]).all(dim=1).nonzero().flatten()
        assert torch.equal(rows[lims[q] : lims[q + 1]], same), q
    assert int(counts[zero].sum()) >= 2 * (nq // 16)


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_nonfinite_queries_and_rows(native, dtype):
    n, d, K, nq, nprobe = 3000, 128, 37, 500, 4
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    r2 = _radii(nq, d)
    clean = _range(ix, Q, C, r2, nprobe)
    Qp = Q.clone()
    bad = [3, 9, 244]                                                 # (classes: most of a cluster, everything, everything)
    Qp[3, 5], Qp[9, 0], Qp[244, 127] = float("nan"), float("inf"), float("-inf")
    assert all(int(clean[0][q + 1] - clean[0][q]) > 0 for q in bad)
    lims, rows, d2 = _range(ix, Qp, C, r2, nprobe)
    counts, cc = lims[1:] - lims[:-1], clean[0][1:] - clean[0][:-1]
    keep = torch.ones(nq, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert counts[bad].tolist() == [0, 0, 0] and torch.equal(counts[keep], cc[keep])
    kq = torch.repeat_interleave(keep, cc)
    assert torch.equal(rows, clean[1][kq]) and torch.equal(_bits(d2), _bits(clean[2][kq]))
    assert torch.equal(ops.index_range(ix, Qp, C, r2, nprobe, count_only=True), counts)
    # rows with a non-finite coordinate are in no list: never returned, whatever the radius
    Xp = X.clone()
    Xp[7], Xp[11, 2], Xp[2999, 64] = float("inf"), float("nan"), float("-inf")
    ixp = ops.index_build(Xp, C)
    big = torch.full((nq,), 1e6 * d, device=DEV)
    o = _Oracle(Q, Xp, C, big, K)
    got = _range(ixp, Q, C, big, K)
    _assert_bitwise(got, o.lims, o.rows, o.d2)
    assert bool((got[0][1:] - got[0][:-1] == n - 3).all()) and not ({7, 11, 2999} & set(got[1][: n].tolist()))
    assert not bool(torch.isin(got[1], torch.tensor([7, 11, 2999], device=DEV)).any())


@pytest.mark.parametrize("dtype", DTYPES)
def test_range_blocking_counts_and_limits(native, dtype):
    n, d, K, nq, nprobe = 513, 30, 7, 17, 3
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    r2 = _radii(nq, d)
    for sort in (True, False):
        whole = ops.index_range(ix, Q, C, r2, nprobe, sort=sort)
        parts = ops.index_range(ix, Q, C, r2, nprobe, sort=sort, block_queries=7)
        assert torch.equal(whole[0], parts[0]) and torch.equal(whole[1], parts[1])
    counts = ops.index_range(ix, Q, C, r2, nprobe, count_only=True, block_queries=7)
    assert counts.dtype == torch.int64 and torch.equal(counts, whole[0][1:] - whole[0][:-1])
    km = mikmeans.KMeans(K, dtype=str(dtype).replace("torch.", ""))
    km.cluster_centers_ = C
    cix = km.build_index(X)
    lims, rows, sq = cix.range_search(Q, r2, nprobe=nprobe, squared=True)
    srt = ops.index_range(ix, Q, C, r2, nprobe)
    assert lims.dtype == rows.dtype == torch.int64 and sq.dtype == torch.float32
    assert torch.equal(lims, srt[0]) and torch.equal(rows, ops.index_decode(srt[1])[0])
    cnt = cix.range_count(Q, r2, nprobe=nprobe, squared=True)
    assert cnt.dtype == torch.int64 and torch.equal(cnt, lims[1:] - lims[:-1])
    # an unsquared radius is squared in float32; the distances are the square roots
    r = r2.sqrt()
    l2, rows2, dist = cix.range_search(Q, r, nprobe=nprobe)
    e = ops.index_range(ix, Q, C, r * r, nprobe)
    assert torch.equal(l2, e[0]) and torch.equal(rows2, ops.index_decode(e[1])[0])
    assert torch.equal(dist, ops.index_decode(e[1])[1].sqrt())
    total = int(lims[-1])
    assert total > 0 and int(cix.range_search(Q, r2, nprobe=nprobe, squared=True, max_results=total)[0][-1]) == total
    with pytest.raises(ValueError, match=str(total)):
        cix.range_search(Q, r2, nprobe=nprobe, squared=True, max_results=total - 1)
    for radius in (-1.0, float("nan"), float("inf"), torch.ones(nq - 1), torch.ones(nq, 1), -r2 - 1.0):
        with pytest.raises(ValueError):
            cix.range_search(Q, radius, nprobe=nprobe)
        with pytest.raises(ValueError):
            cix.range_count(Q, radius, nprobe=nprobe)
    for bad in (0, K + 1):
        with pytest.raises(ValueError):
            cix.range_search(Q, 1.0, nprobe=bad)
        with pytest.raises(ValueError):
            cix.range_count(Q, 1.0, nprobe=bad)
        with pytest.raises(ValueError):
            ops.index_range(ix, Q, C, 1.0, bad)
    with pytest.raises(ValueError):
        cix.range_search(Q[0], 1.0, nprobe=nprobe)
    with pytest.raises(ValueError):
        ops.index_range(ix, Q[0], C, 1.0, nprobe)


def test_estimator_range_search(native):
    n, d, K, nq, nprobe = 3000, 128, 37, 500, 4
    X, C, Q, _ = _data(n, d, K, torch.bfloat16, nq)
    r2 = _radii(nq, d)
    o = _Oracle(Q, X, C, r2, nprobe)
    km = mikmeans.KMeans(K, dtype="bfloat16")
    km.cluster_centers_ = C
    ix = km.build_index(X)
    got = ix.range_search(Q, r2, nprobe=nprobe, squared=True)
    _assert_bitwise(got, o.lims, o.rows, o.d2)
    _assert_bitwise(ix.range_search(Q, r2, nprobe=nprobe, squared=True, sort=False), o.lims, o.urows, o.ud2)
    # host rows in small blocks build the same index; numpy queries in, numpy out
    host = km.build_index(X.float().cpu().numpy(), block_rows=777)
    nl, nr, nd = host.range_search(Q.float().cpu().numpy(), r2.cpu().numpy(), nprobe=nprobe, squared=True)
    assert all(isinstance(t, np.ndarray) for t in (nl, nr, nd))
    assert nl.dtype == nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nl, o.lims.cpu().numpy()) and np.array_equal(nr, o.rows.cpu().numpy())
    assert np.array_equal(nd, o.d2.cpu().numpy())
    nc = host.range_count(Q.float().cpu().numpy(), r2.cpu().numpy(), nprobe=nprobe, squared=True)
    assert isinstance(nc, np.ndarray) and nc.dtype == np.int64 and np.array_equal(nc, np.diff(nl))
    none = km.build_index(X[:0])                                       # no rows: no hits
    zl, zr, zd = none.range_search(Q[:40], 1e3, nprobe=nprobe)
    assert zl.shape == (41,) and bool((zl == 0).all()) and zr.numel() == 0 and zd.numel() == 0
    assert zr.dtype == torch.int64 and zd.dtype == torch.float32
    assert bool((none.range_count(Q[:40], 1e3, nprobe=nprobe) == 0).all())
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, dtype="bfloat16", seed=0).fit(X)
    om = _Oracle(Q, X, mb.cluster_centers_, r2, 8)
    _assert_bitwise(mb.build_index(X).range_search(Q, r2, nprobe=8, squared=True), om.lims, om.rows, om.d2)


def test_the_range_mirror_agrees_on_exact_data(native):
    """The CPU mirror and the kernels on small-integer rows (every distance exact): one answer; rows
    wider than the kernels take the mirror on the device."""
    g = torch.Generator().manual_seed(3)
    X = torch.randint(-3, 4, (900, 20), generator=g).float()
    C = torch.randint(-3, 4, (11, 20), generator=g).float()
    Q = torch.randint(-3, 4, (60, 20), generator=g).float()
    r2 = torch.tensor([0.0, 60.0, 90.0, 120.0, 1e6])[torch.arange(60) % 5]
    cpu_ix = ops.index_build(X, C)
    gpu_ix = ops.index_build(X.to(DEV), C.to(DEV))
    assert not cpu_ix.native and gpu_ix.native
    for sort in (True, False):
        el, ek = ref.index_range(cpu_ix, Q, C, r2, 3, sort=sort)
        gl, gk = ops.index_range(gpu_ix, Q.to(DEV), C.to(DEV), r2.to(DEV), 3, sort=sort)
        assert int(el[-1]) > 60 and torch.equal(gl.cpu(), el) and torch.equal(gk.cpu(), ek)
    half = torch.randint(-3, 4, (150, 1100), generator=g).float()
    Xw, Cw = torch.cat([half, half]).to(DEV), torch.randint(-3, 4, (4, 1100), generator=g).float().to(DEV)
    Qw = torch.randint(-3, 4, (20, 1100), generator=g).float().to(DEV)
    wix = ops.index_build(Xw, Cw)
    assert not wix.native and wix.pack.is_cuda
    exact = (torch.cdist(Qw.double(), Xw.double()) ** 2).round()
    rw = exact.sort(dim=1).values[:, 5].float()                       # the 6th smallest distance
    lims, keys = ops.index_range(wix, Qw, Cw, rw, 4)
    rows, d2 = ops.index_decode(keys)
    hit = exact <= rw[:, None].double()
    sv, si = torch.sort(torch.where(hit, exact, float("inf")), dim=1, stable=True)
    ok = torch.arange(300, device=DEV)[None, :] < hit.sum(1)[:, None]
    assert keys.is_cuda and torch.equal(lims[1:] - lims[:-1], hit.sum(1)) and int(lims[-1]) >= 120
    assert torch.equal(rows, si[ok]) and torch.equal(d2.double(), sv[ok])
