"""build_index / search on the GPU (csrc/ivf.hip): the native partition against the stable sort,
the row pack against pack_centers list by list, and the search bit for bit against an oracle built
from the existing kernels only -- transform(Q, X.float(), squared=True), the columns outside the
probed lists masked out, a stable sort over (value, row id).  (The CPU mirrors: test_ivf.py.)"""
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


# ---------------------------------------------------------------------------- partition
def _stable(labels, K):
    lab = labels.long()
    rows = ((lab >= 0) & (lab < K)).nonzero().flatten()
    order = torch.full_like(lab, -1)
    order[: rows.numel()] = rows[torch.sort(lab[rows], stable=True).indices]
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=lab.device)
    offsets[1:] = torch.cumsum(torch.bincount(lab[rows], minlength=K), 0)
    return order, offsets


def _labels(kind, n, K):
    g = torch.Generator().manual_seed(n + K)
    if kind == "one":
        return torch.full((n,), K // 2, dtype=torch.int32)
    lab = torch.randint(0, K, (n,), generator=g, dtype=torch.int32)
    if kind == "invalid":
        lab[torch.randint(0, n, (n // 7 + 1,), generator=g)] = -1
        lab[torch.randint(0, n, (n // 9 + 1,), generator=g)] = K
        lab[0], lab[n - 1] = K + 5, -3
    return lab


# (kind, n, K): one row; a ragged wave on either side of 64; several waves and workgroups; the
# largest LDS tables; a K past the native bound (the stable torch.sort); every row in one label;
# labels outside [0, K); more labels than rows
PARTITIONS = [("rand", 1, 1), ("rand", 63, 3), ("rand", 64, 3), ("rand", 65, 3), ("rand", 5000, 37),
              ("rand", 70001, 1024), ("rand", 200003, 4097), ("rand", 5000, ops.PARTITION_MAX_K),
              ("rand", 5000, ops.PARTITION_MAX_K + 1), ("one", 3001, 9), ("invalid", 5000, 37), ("rand", 10, 100)]


@pytest.mark.parametrize("kind,n,K", PARTITIONS)
def test_partition_is_the_stable_sort(native, kind, n, K):
    lab = _labels(kind, n, K).to(DEV)
    eo, eoff = _stable(lab, K)
    order, offsets, rpos = ops.partition(lab, K, want_pos=True)
    assert order.dtype == offsets.dtype == torch.int64 and order.shape == (n,) and offsets.shape == (K + 1,)
    assert torch.equal(offsets, eoff) and torch.equal(order, eo)
    nv = int(offsets[-1])
    assert torch.equal(rpos[order[:nv]], torch.arange(nv, device=DEV)) and int((rpos >= 0).sum()) == nv
    again = ops.partition(lab, K)
    assert torch.equal(again[0], order) and torch.equal(again[1], offsets)


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


def _lists(X, C):
    idx, d2 = ops.topk(X, C, 1)
    return torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1).long()


def _oracle(Q, X, C, m, nprobe):
    """(rows, d2) from the existing kernels: the transform kernel's distances with the rows as
    centres, restricted to the probed lists, in a stable sort (equal values by row id)."""
    K, nq = C.shape[0], Q.shape[0]
    lab = _lists(X, C)
    probes = ops.topk(Q, C, nprobe)[0].long()
    member = torch.zeros((nq, K + 1), dtype=torch.bool, device=DEV)
    member.scatter_(1, probes, True)
    allowed = member[:, torch.where(lab < 0, K, lab)]
    Dm = ops.transform(Q, X.float(), squared=True)
    sv, si = torch.sort(torch.where(allowed, Dm, float("inf")), dim=1, stable=True)
    ok = torch.arange(m, device=DEV)[None, :] < allowed.sum(1)[:, None]
    return torch.where(ok, si[:, :m], -1), torch.where(ok, sv[:, :m], float("nan"))


def _search(index, Q, C, m, nprobe):
    return ops.index_decode(ops.index_search(index, Q, C, m, nprobe))


def _assert_bitwise(got, exp):
    (rows, d2), (er, ed) = got, exp
    assert rows.dtype == torch.int64 and d2.dtype == torch.float32 and rows.shape == d2.shape == er.shape
    assert torch.equal(rows, er), int((rows != er).sum())
    assert torch.equal(d2.view(torch.int32), ed.view(torch.int32)), int((d2.view(torch.int32) != ed.view(torch.int32)).sum())


@functools.lru_cache(maxsize=None)
def _index(n, d, K, dtype, nq):
    X, C, _, _ = _data(n, d, K, dtype, nq)
    return ops.index_build(X, C)


# ------------------------------------------------------------------------------ build
BUILDS = [(3000, 128, 37), (513, 30, 7), (1200, 300, 20), (700, 1024, 5)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K", BUILDS)
def test_index_lists_and_row_pack(native, dtype, n, d, K):
    X, C, _, sizes = _data(n, d, K, dtype, 64)
    ix = _index(n, d, K, dtype, 64)
    assert ix.native and torch.equal(ix.offsets[1:] - ix.offsets[:-1], sizes)
    eo, eoff = _stable(_lists(X, C), K)
    assert torch.equal(ix.order, eo) and torch.equal(ix.offsets, eoff)
    Xp = ops.pad_columns(X)
    bits = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert ix.pack.numel() == ops.index_tiles(n, K) * 16 * ix.cols and ix.cn.numel() == ops.index_tiles(n, K) * 16
    for k in range(K):
        a, b = int(ix.offsets[k]), int(ix.offsets[k + 1])
        rows = ix.order[a:b]
        assert bool((rows[1:] > rows[:-1]).all())                     # ascending within the list
        if b == a:
            assert int(ix.tile_offsets[k + 1]) == int(ix.tile_offsets[k])
            continue
        pk = ops.pack_centers(Xp[rows].float(), Xp.shape[1], dtype, DEV)
        assert pk.dpad == ix.cols
        t0, nt = int(ix.tile_offsets[k]), (b - a + 15) // 16
        assert int(ix.tile_offsets[k + 1]) == t0 + nt
        seg = ix.pack[t0 * 16 * ix.cols : (t0 + nt) * 16 * ix.cols]
        assert torch.equal(seg.view(bits), pk.pack[: nt * 16 * ix.cols].view(bits)), k
        assert torch.equal(ix.cn[t0 * 16 : (t0 + nt) * 16].view(torch.int32), pk.cn[: nt * 16].view(torch.int32)), k
    for other in (ops.index_build(X, C, block_rows=777), ops.index_build(X, C)):   # any blocking, any run
        for name, t in ix.tensors().items():
            assert torch.equal(t.view(torch.uint8), other.tensors()[name].view(torch.uint8)), name


# ----------------------------------------------------------------------------- search
# (n, D, K, nq, m, nprobe): the base shape with the short list, one slot and the long list, one probe
# and every list (the exact search); D -> DPAD 32 with m past the short list; ragged wide rows; DPAD
# 1024; many short lists (whole lists inside one tile); one query; pair counts past the launcher's
# small-batch rule, which run 4 | 3 (m = 8) and 2 | 1 (m = 32) pair blocks a wave
SEARCHES = [(3000, 128, 37, 500, 8, 4), (3000, 128, 37, 500, 1, 4), (3000, 128, 37, 500, 32, 4),
            (3000, 128, 37, 500, 8, 1), (3000, 128, 37, 500, 8, 37), (513, 30, 7, 17, 9, 3),
            (1200, 300, 20, 65, 16, 5), (700, 1024, 5, 33, 8, 2), (20011, 64, 1024, 300, 8, 16),
            (3000, 128, 37, 1, 8, 4), (3000, 128, 37, 8200, 8, 16), (3000, 128, 37, 4100, 32, 16)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,m,nprobe", SEARCHES)
def test_search_is_the_masked_sorted_transform_bitwise(native, dtype, n, d, K, nq, m, nprobe):
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    ix = _index(n, d, K, dtype, nq)
    got = _search(ix, Q, C, m, nprobe)
    _assert_bitwise(got, _oracle(Q, X, C, m, nprobe))
    again = _search(ix, Q, C, m, nprobe)
    assert torch.equal(again[0], got[0]) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_lists_probed_by_few_and_many_queries(native, dtype):
    """One probe per query, the queries placed on chosen centres: lists probed by 1, 16, 17 and 70
    queries (one pair, a full block, a block and one, five blocks) and a list nobody probes."""
    n, d, K = 3000, 128, 37
    X, C, _, _ = _data(n, d, K, dtype, 64)
    ix = _index(n, d, K, dtype, 64)
    want = {6: 1, 9: 16, 12: 17, 20: 70}
    g = torch.Generator().manual_seed(5)
    Q = torch.cat([C[k].cpu() + 0.25 * torch.randn(c, d, generator=g) for k, c in want.items()])
    Q = Q[torch.randperm(Q.shape[0], generator=g)].to(dtype).to(DEV)
    probed = torch.bincount(ops.topk(Q, C, 1)[0][:, 0].long(), minlength=K)
    assert {k: int(probed[k]) for k in want} == want and int(probed.sum()) == sum(want.values())
    _assert_bitwise(_search(ix, Q, C, 8, 1), _oracle(Q, X, C, 8, 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_search_pads_short_lists(native, dtype):
    """Queries on the centres of the empty list and of the lists of 1 and 15 rows, one probe: fewer
    than m = 16 candidates, padded with (-1, NaN); the other queries find full lists."""
    n, d, K, m = 3000, 128, 37, 16
    X, C, Qn, sizes = _data(n, d, K, dtype, 64)
    ix = _index(n, d, K, dtype, 64)
    assert sizes[:3].tolist() == [0, 1, 15]
    Q = torch.cat([C[:3].to(dtype), Qn])
    rows, d2 = _search(ix, Q, C, m, 1)
    _assert_bitwise((rows, d2), _oracle(Q, X, C, m, 1))
    found = (rows >= 0).sum(1)
    assert found[:3].tolist() == [0, 1, 15]
    assert bool((rows[1, 1:] == -1).all()) and bool(d2[1, 1:].isnan().all()) and bool(d2[0].isnan().all())
    padded = found < m
    assert int(padded.sum()) >= 1 and float((~padded).float().mean()) >= 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,m", [(1400, 24, 10, 300, 8), (1400, 24, 10, 300, 32), (600, 300, 6, 70, 16)])
def test_search_exact_ties_go_to_the_lower_row(native, dtype, n, d, K, nq, m):
    """Small integers (exact in bf16 and in the f32 accumulation) with rows i and i + n/2 identical:
    every query's nearest row has a twin at the same distance, listed behind it."""
    g = torch.Generator().manual_seed(n + m)
    half = torch.randint(-3, 4, (n // 2, d), generator=g).float()
    X = torch.cat([half, half]).to(dtype).to(DEV)
    C = torch.randint(-3, 4, (K, d), generator=g).float().to(DEV)
    Q = torch.randint(-3, 4, (nq, d), generator=g).to(dtype).to(DEV)
    ix = ops.index_build(X, C)
    rows, d2 = _search(ix, Q, C, m, K)
    _assert_bitwise((rows, d2), _oracle(Q, X, C, m, K))
    tie = d2[:, 1:] == d2[:, :-1]
    assert bool((rows[:, 1:][tie] > rows[:, :-1][tie]).all())
    assert float(tie.any(dim=1).float().mean()) >= 0.5             # (every query: its nearest row has a twin)
    Qd, Xd = Q.double(), X.double()                                # (integers: every f64 operation is exact)
    exact = (Qd * Qd).sum(1)[:, None] + (Xd * Xd).sum(1)[None, :] - 2 * (Qd @ Xd.T)
    assert torch.equal(d2.double(), exact.gather(1, rows))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K,nq,m", [(3000, 128, 37, 500, 8), (513, 30, 7, 17, 9), (1200, 300, 20, 65, 16),
                                        (700, 1024, 5, 33, 8)])
def test_exact_search_against_float64(native, dtype, n, d, K, nq, m):
    """nprobe = K is the brute-force search: against float64 distances under the tolerance of
    test_topk_against_float64 (the same arithmetic, rows in the place of centres)."""
    X, C, Q, _ = _data(n, d, K, dtype, nq)
    rows, d2 = _search(_index(n, d, K, dtype, nq), Q, C, m, K)
    Xq, Qc = X.cpu().double(), Q.cpu().double()
    exp = torch.cdist(Qc, Xq)
    tol = (3e-5 if dtype == torch.float32 else 1e-4) * (Qc.norm(dim=1, keepdim=True) + Xq.norm(dim=1).max()) + 1e-3
    best = exp.sort(dim=1).values[:, :m]
    err = (d2.cpu().double().sqrt() - best).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    true = exp.gather(1, rows.cpu())
    assert bool((true <= best[:, -1:] + 2 * tol).all()), float((true - best[:, -1:] - 2 * tol).max())


# -------------------------------------------------------------------------- estimator
def test_estimator_build_index_and_search(native):
    n, d, K, nq = 3000, 128, 37, 500
    X, C, Q, sizes = _data(n, d, K, torch.bfloat16, nq)
    km = mikmeans.KMeans(K, dtype="bfloat16")
    km.cluster_centers_ = C
    ix = km.build_index(X)
    assert isinstance(ix, mikmeans.ClusterIndex) and ix.n_rows == n and torch.equal(ix.list_sizes, sizes)
    assert torch.equal(ix.rows_of(5), ix.order[int(ix.offsets[5]) : int(ix.offsets[6])])
    er, ed = _oracle(Q, X, C, 10, 4)
    rows, d2 = ix.search(Q, 10, nprobe=4, squared=True)
    _assert_bitwise((rows, d2), (er, ed))
    rows, dist = ix.search(Q, 10, nprobe=4)
    assert torch.equal(rows, er) and torch.equal(dist, ed.sqrt())
    # host rows in small blocks build the same index; numpy queries in, numpy out
    host = km.build_index(X.float().cpu().numpy(), block_rows=777)
    for name, t in ix._index.tensors().items():
        assert torch.equal(t.view(torch.uint8), host._index.tensors()[name].view(torch.uint8)), name
    nr, nd = host.search(Q.float().cpu().numpy(), 10, nprobe=4, squared=True)
    assert isinstance(nr, np.ndarray) and isinstance(nd, np.ndarray) and nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nr, er.cpu().numpy()) and np.array_equal(nd, ed.cpu().numpy(), equal_nan=True)
    for bad in ((0, 4), (33, 4), (8, 0), (8, K + 1)):
        with pytest.raises(ValueError):
            ix.search(Q, bad[0], nprobe=bad[1])
    none = km.build_index(X[:0])                                       # no rows: every slot empty
    er0, ed0 = none.search(Q[:40], 3, nprobe=4)
    assert none.order.numel() == 0 and bool((er0 == -1).all()) and bool(ed0.isnan().all())
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, dtype="bfloat16", seed=0).fit(X)
    mr, md = mb.build_index(X).search(Q, 5, nprobe=8, squared=True)
    _assert_bitwise((mr, md), _oracle(Q, X, mb.cluster_centers_, 5, 8))


def test_build_index_refuses_what_does_not_fit(native, monkeypatch):
    from mikmeans.parallel import memplan

    X, C, _, _ = _data(3000, 128, 37, torch.bfloat16, 64)
    km = mikmeans.KMeans(37, dtype="bfloat16")
    km.cluster_centers_ = C
    plan = memplan.plan_index(3000, 128, 37, "bfloat16")
    ix = _index(3000, 128, 37, torch.bfloat16, 64)
    assert {k: memplan._r(t.numel() * t.element_size()) for k, t in ix.tensors().items()} == plan.persistent
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", str(plan.peak - 1))
    with pytest.raises(memplan.HBMCapacityError):
        km.build_index(X)
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", str(plan.peak))
    assert km.build_index(X).nbytes == ix.nbytes


def test_rows_wider_than_the_kernels_take_the_mirror(native):
    """D > 1024: the torch mirror on the device (small integers: every distance exact), against the
    exact float64 distances in a stable sort."""
    g = torch.Generator().manual_seed(9)
    half = torch.randint(-3, 4, (150, 1100), generator=g).float()
    X, C = torch.cat([half, half]).to(DEV), torch.randint(-3, 4, (4, 1100), generator=g).float().to(DEV)
    Q = torch.randint(-3, 4, (20, 1100), generator=g).float().to(DEV)
    ix = ops.index_build(X, C)
    assert not ix.native and ix.pack.is_cuda and int(ix.offsets[-1]) == 300
    rows, d2 = _search(ix, Q, C, 6, 4)
    exact = torch.cdist(Q.double(), X.double()) ** 2
    sv, si = torch.sort(exact.round(), dim=1, stable=True)
    assert torch.equal(rows, si[:, :6]) and torch.equal(d2.double(), sv[:, :6])


def test_the_mirror_agrees_on_exact_data(native):
    """The CPU mirror and the kernels on small-integer rows (every distance exact): one answer."""
    g = torch.Generator().manual_seed(3)
    X = torch.randint(-3, 4, (900, 20), generator=g).float()
    C = torch.randint(-3, 4, (11, 20), generator=g).float()
    Q = torch.randint(-3, 4, (60, 20), generator=g).float()
    cpu_ix = ops.index_build(X, C)
    gpu_ix = ops.index_build(X.to(DEV), C.to(DEV))
    assert not cpu_ix.native and gpu_ix.native
    assert torch.equal(cpu_ix.order, gpu_ix.order.cpu()) and torch.equal(cpu_ix.offsets, gpu_ix.offsets.cpu())
    assert torch.equal(ref.index_search(cpu_ix, Q, C, 8, 3), ops.index_search(gpu_ix, Q.to(DEV), C.to(DEV), 8, 3).cpu())


# ------------------------------------------------------------------- the binding's checks
def test_the_binding_refuses_a_wrong_walk(native):
    """ivf_scan and ivf_range with the arguments ops.pair_items gives, one of them wrong at a time:
    a P that is neither 1 nor the rule's, max_items one below and one above the accepted window
    (from the full blocks alone, npairs // 16 P, to K + 1 above that), a pack that is not whole
    tiles, a porder shorter than the pairs and an int32 icum are refused on the host (RuntimeError,
    before any launch); the unmodified calls then give ops.index_search / ops.index_range."""
    from mikmeans.ops.native import dtype_code, require

    ext = require()
    n, d, K, nq, nprobe, m = 70, 16, 3, 5, 2, 4
    g = torch.Generator().manual_seed(70)
    C = 8.0 * torch.randn(K, d, generator=g)
    lab = torch.repeat_interleave(torch.arange(K), torch.tensor([0, 17, 53]))[torch.randperm(n, generator=g)]
    X = (C[lab] + 0.25 * torch.randn(n, d, generator=g)).to(DEV)
    Q = (X[torch.randint(0, n, (nq,), generator=g).to(DEV)].cpu() + 0.25 * torch.randn(nq, d, generator=g)).to(DEV)
    C = C.to(DEV)
    ix = ops.index_build(X, C)
    assert ix.native and (ix.offsets[1:] - ix.offsets[:-1]).tolist() == [0, 17, 53]
    probes, npairs, code = ops.topk(Q, C, nprobe)[0], nq * nprobe, dtype_code(torch.float32)
    r2 = torch.full((nq,), 3.0, device=DEV)

    def refusals(op, P, lead, tail):
        porder, poff, icum, max_items = ops.pair_items(ix, probes, P)
        good = [*lead, ix.pack, ix.cn, ix.offsets, ix.tile_offsets, ix.order, porder, poff, icum, nprobe, ix.cols, P,
                max_items]
        i_pack, i_porder, i_icum, i_P, i_max = (len(lead) + i for i in (0, 5, 7, 10, 11))
        assert good[i_pack] is ix.pack and good[i_porder] is porder and good[i_icum] is icum and good[i_P] == P == 1
        lo = npairs // (16 * P)
        assert lo <= max_items <= lo + K + 1
        for i, bad in ((i_P, 2), (i_max, lo - 1), (i_max, lo + K + 2), (i_pack, ix.pack[:-1]), (i_porder, porder[:-1]),
                       (i_icum, icum.to(torch.int32))):
            args = list(good)
            args[i] = bad
            with pytest.raises(RuntimeError):
                op(*args, *tail)
        op(*good, *tail)
        return good

    qn = ops.row_sqnorm(Q)
    out = torch.empty((npairs, m), dtype=torch.int64, device=DEV)
    refusals(ext.ivf_scan, ext.ivf_scan_blocks(code, ix.cols, m, npairs), [Q, qn], [out])
    assert torch.equal(out.view(nq, nprobe * m).sort(dim=1).values[:, :m], ops.index_search(ix, Q, C, m, nprobe))

    counts = torch.zeros(npairs, dtype=torch.int64, device=DEV)
    good = refusals(ext.ivf_range, ext.ivf_range_blocks(code, ix.cols, npairs), [Q, qn, r2], [counts])
    lims, ekeys = ops.index_range(ix, Q, C, r2, nprobe, sort=False)
    end = torch.cumsum(counts, 0)
    assert int(end[-1]) == ekeys.numel() > 0 and torch.equal(end.view(nq, nprobe)[:, -1], lims[1:])
    keys = torch.empty(int(end[-1]), dtype=torch.int64, device=DEV)
    ext.ivf_range(*good, counts, end - counts, keys)
    assert torch.equal(keys, ekeys)
