"""The product-quantised index on the GPU: the scan of csrc/pq.hip against an oracle made of the
existing kernels (top-k, transform) and torch elementwise ops on the device, the splits and the
query blocking, the layout, the training and the public interface.  Every comparison is bitwise.

The data has thirteen lists: the twelve prescribed sizes 0, 1, 15, 16, 17, 33, 63, 64, 65, 255, 256
and 257 (each needs a centre of its own, the empty one too) and one more list of 2100 rows, longer
than 8 splits x 256 rows, with 40 copies of one row in it -- so ``K`` is 13, one more than a round
dozen."""
import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 15, 16, 17, 33, 63, 64, 65, 255, 256, 257, 2100]
K = len(SIZES)
LONG, COPIES, NQ = K - 1, 40, 37
EMPTY = ops.IVF_EMPTY_KEY
SHAPES = [(8, 8), (64, 16), (128, 32), (128, 64)]


def _name(dtype):
    return "bfloat16" if dtype == torch.bfloat16 else "float32"


class Case:
    """One (F, M, dtype): rows, centres, given codebooks, the index and the oracle's pieces."""

    def __init__(self, F, M, dtype, dev="cuda:0"):
        dev = torch.device(dev)
        g = torch.Generator().manual_seed(1000 * F + M)
        self.F, self.M, self.dtype, self.dev = F, M, dtype, dev
        # well-separated centres: 13 corners of a cube of side 40 (noise 1 per coordinate)
        C = torch.zeros(K, F)
        for k in range(K):
            for b in range(4):
                C[k, b::4] = 40.0 * ((k >> b) & 1)
        C += torch.randn(K, F, generator=g)
        lab = torch.repeat_interleave(torch.arange(K), torch.tensor(SIZES))
        X = C[lab] + torch.randn(lab.numel(), F, generator=g)
        long_rows = (lab == LONG).nonzero().flatten()
        X[long_rows[:COPIES]] = X[long_rows[COPIES]].clone()               # 40 rows that are copies of one row
        perm = torch.randperm(X.shape[0], generator=g)
        X, lab = X[perm], lab[perm]
        self.copy_ids = (perm[:, None] == long_rows[None, : COPIES + 1]).any(1).nonzero().flatten().to(dev)
        self.C = C.to(dev)
        self.X = X.to(dev).to(dtype)
        self.n = X.shape[0]
        # queries near rows: every list but the empty one, the copies' row among them; and the centres
        # of the 0-, 1- and 15-row lists
        pick = torch.cat([perm.argsort()[long_rows[COPIES : COPIES + 1]], torch.randperm(self.n, generator=g)[: NQ - 4]])
        Q = torch.cat([X[pick] + 0.1 * torch.randn(NQ - 3, F, generator=g), C[:3] + 0.1])
        self.Q = Q.to(dev).to(dtype)
        assert self.Q.shape[0] == NQ
        # the lists and the residuals, by the existing kernels
        self.lab = ops.topk(self.X, self.C, 1)[0][:, 0].long()
        assert torch.equal(self.lab.cpu(), lab)
        self.R = (self.X.float() - self.C[self.lab]).to(dtype)
        dsub = F // M
        rows = torch.randperm(self.n, generator=g)[:256].to(dev)
        self.books = self.R[rows].float().view(256, M, dsub).permute(1, 0, 2).contiguous()
        self.codes = ops.pq_encode(self.R, self.books)
        self.index = ops.pq_build(self.X, self.C, M, codebooks=self.books)
        self._oracle = {}

    def oracle(self, nprobe):
        """Sorted keys int64 [NQ, n] over all rows (EMPTY behind the rows of the probed lists): probes by
        ops.topk, tables by ops.transform per sub-space, the per-row sum a loop of M torch.adds in
        order, rows outside the probed lists masked, a stable sort by (value, row)."""
        if nprobe in self._oracle:
            return self._oracle[nprobe]
        F, M, dsub, dev = self.F, self.M, self.F // self.M, self.dev
        probes = ops.topk(self.Q, self.C, nprobe)[0].long()                     # [NQ, nprobe]
        RQ = (self.Q.float()[:, None, :] - self.C[probes]).to(self.dtype).view(NQ * nprobe, F)
        lut = torch.stack([ops.transform(RQ[:, j * dsub : (j + 1) * dsub].contiguous(), self.books[j], squared=True)
                           for j in range(M)], dim=1)                           # [npairs, M, 256]
        assert bool((lut >= 0).all())
        rank = torch.full((NQ, K), -1, dtype=torch.int64, device=dev)
        rank.scatter_(1, probes, torch.arange(nprobe, device=dev)[None, :].expand(NQ, nprobe))
        of = rank[:, self.lab]                                                  # [NQ, n]: rows in natural order
        pair = torch.arange(NQ, device=dev)[:, None] * nprobe + of.clamp(min=0)
        c = self.codes.long()
        acc = lut[pair, 0, c[None, :, 0]]
        for j in range(1, M):
            acc = torch.add(acc, lut[pair, j, c[None, :, j]])
        val = torch.where(of >= 0, acc, float("inf"))
        v, rows = torch.sort(val, dim=1, stable=True)                           # (rows ascending among equal values)
        keys = (v.contiguous().view(torch.int32).to(torch.int64) << 32) | rows
        keys = torch.where(torch.isinf(v), EMPTY, keys)
        self._oracle[nprobe] = (keys, probes)
        return self._oracle[nprobe]


_cases = {}


@pytest.fixture(params=[(F, M, dt) for F, M in SHAPES for dt in (torch.bfloat16, torch.float32)],
                ids=lambda p: f"F{p[0]}-M{p[1]}-{_name(p[2])}")
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(*request.param)
    return _cases[request.param]


def _eq(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("nprobe", [1, 3, K])
def test_scan_against_the_oracle(case, nprobe):
    want, probes = case.oracle(nprobe)
    for m in (1, 8, 9, 16, 17, 32):                                           # (every list length and the cuts between)
        keys = ops.pq_search(case.index, case.Q, case.C, m, nprobe)
        assert keys.dtype == torch.int64
        assert _eq(keys, want[:, :m]), (m, nprobe)
    if nprobe == 1:
        keys = ops.pq_search(case.index, case.Q, case.C, 32, 1)
        for q, size in ((NQ - 3, 0), (NQ - 2, 1), (NQ - 1, 15)):              # nearest the 0- / 1- / 15-row lists
            assert int(probes[q, 0]) == SIZES.index(size)
            assert int((keys[q] != EMPTY).sum()) == size and bool((keys[q, size:] == EMPTY).all())
    # the copies: one distance on 41 rows, in ascending row order
    if nprobe == K:
        keys = ops.pq_search(case.index, case.Q, case.C, 32, nprobe)
        rows, d2 = ops.index_decode(keys)
        first = rows[0, : COPIES + 1 if COPIES + 1 <= 32 else 32]
        assert torch.equal(first, case.copy_ids[: first.numel()]) and bool((d2[0, : first.numel()] == d2[0, 0]).all())


def test_splits_blocking_and_repeats(case):
    m, nprobe = 9, 3
    want = case.oracle(nprobe)[0][:, :m]
    for splits in (1, 2, 8):
        assert _eq(ops.pq_search(case.index, case.Q, case.C, m, nprobe, splits=splits), want), splits
    for block in (5, 16):
        assert _eq(ops.pq_search(case.index, case.Q, case.C, m, nprobe, block_queries=block), want), block
    for q in (0, 11, NQ - 1):
        assert _eq(ops.pq_search(case.index, case.Q[q : q + 1], case.C, m, nprobe), want[q : q + 1]), q
    a = ops.pq_search(case.index, case.Q, case.C, 32, K, splits=8)
    assert _eq(a, ops.pq_search(case.index, case.Q, case.C, 32, K, splits=8))
    assert _eq(a, case.oracle(K)[0][:, :32])


def test_layout(case):
    ix, n, M = case.index, case.n, case.M
    flat = ops.index_build(case.X, case.C)
    assert torch.equal(ix.order, flat.order) and torch.equal(ix.offsets, flat.offsets)
    assert ix.codes.dtype == torch.uint8 and ix.codes.shape == (n, M) and ix.codes.is_contiguous()
    assert ix.codes.data_ptr() % 16 == 0
    assert (ix.offsets[1:] - ix.offsets[:-1]).tolist() == SIZES
    for l in range(K):
        a, b = int(ix.offsets[l]), int(ix.offsets[l + 1])
        assert torch.equal(ix.codes[a:b], case.codes[ix.order[a:b]]), l
    dsub = case.F // M
    assert ix.nbytes == n * M + 8 * n + 8 * (K + 1) + 4 * M * 256 * dsub
    other = ops.pq_build(case.X, case.C, M, codebooks=case.books, block_rows=1000)
    for a, b in zip(ix.tensors().values(), other.tensors().values()):
        assert torch.equal(a, b)
    # rows with a NaN or inf coordinate are in no list and leave every other row's codes unchanged
    X2 = case.X.clone()
    bad = torch.tensor([3, 500, n - 1], device=case.dev)
    X2[bad[0], 0] = float("nan")
    X2[bad[1], case.F - 1] = float("inf")
    X2[bad[2], 1] = float("-inf")
    ix2 = ops.pq_build(X2, case.C, M, codebooks=case.books)
    nv = int(ix2.offsets[-1])
    assert nv == n - 3 and not bool(torch.isin(ix2.order, bad).any())
    assert bool((ix2.order[nv:] == -1).all()) and bool((ix2.codes[nv:] == 0).all())
    assert torch.equal(ix2.codes[:nv], case.codes[ix2.order[:nv]])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
def test_training(dtype):
    case = _cases.get((64, 16, dtype)) or Case(64, 16, dtype)
    _cases[(64, 16, dtype)] = case
    M, dsub = 8, 8
    R = case.R
    a = ops.pq_train(R, M, max_iter=8, seed=5)
    b = ops.pq_train(R, M, max_iter=8, seed=5)
    assert a.shape == (M, 256, dsub) and a.dtype == torch.float32 and torch.equal(a, b)

    def mse(books):
        codes = ops.pq_encode(R, books).long()
        rec = books[torch.arange(M, device=R.device)[None, :], codes].reshape(R.shape[0], -1)
        return float(((rec.double() - R.double()) ** 2).sum(1).mean())

    first = R[:256].float().view(256, M, dsub).permute(1, 0, 2).contiguous()
    e_trained, e_first = mse(a), mse(first)
    print(f"quantisation error: trained {e_trained:.5f}, first 256 rows {e_first:.5f}")
    assert e_trained < e_first
    with pytest.raises(ValueError, match="at least 256"):
        ops.pq_train(R[:255], M)


def test_api(case, tmp_path):
    dtype, M, F = case.dtype, case.M, case.F
    km = mikmeans.KMeans(K, dtype=_name(dtype), device=case.dev)
    km.cluster_centers_ = case.C.clone()
    ix = km.build_pq_index(case.X, M, codebooks=case.books)
    assert isinstance(ix, mikmeans.PQIndex) and ix.n_rows == case.n == ix.n_indexed and ix.n_subvectors == M
    assert ix.nbytes == case.n * M + 8 * case.n + 8 * (K + 1) + 4 * M * 256 * (F // M)
    assert torch.equal(ix._index.codes, case.index.codes) and torch.equal(ix.order, case.index.order)
    keys = ops.pq_search(case.index, case.Q, case.C, 10, 3)
    r0, d0 = ops.index_decode(keys)
    rows, d2 = ix.search(case.Q, 10, nprobe=3, squared=True)
    assert torch.equal(rows, r0) and _eq(d2, d0)
    rows1, d = ix.search(case.Q, 10, nprobe=3)
    assert torch.equal(rows1, rows) and _eq(d, d0.sqrt())
    rn, dn = ix.search(case.Q.float().cpu().numpy(), 10, nprobe=3)
    assert isinstance(rn, np.ndarray) and isinstance(dn, np.ndarray)
    assert np.array_equal(rn, rows.cpu().numpy()) and np.array_equal(dn.view(np.int32), d.cpu().numpy().view(np.int32))
    # padding: row -1 and NaN
    rp, dp = ix.search(case.Q[NQ - 3 :], 32, nprobe=1)
    assert bool((rp[0] == -1).all()) and bool(torch.isnan(dp[0]).all()) and int((rp[1] >= 0).sum()) == 1
    # reconstruct
    ids = torch.tensor([0, 17, case.n - 1], device=case.dev)
    want = case.C[case.lab[ids]] + case.books[torch.arange(M, device=case.dev)[None, :], case.codes[ids].long()].reshape(3, F)
    assert torch.equal(ix.reconstruct(ids), want)
    # save / load
    ix.save(tmp_path / "pq")
    back = km.load_pq_index(tmp_path / "pq")
    r2, d22 = back.search(case.Q, 10, nprobe=3, squared=True)
    assert torch.equal(r2, rows) and _eq(d22, d2)
    other = mikmeans.KMeans(K, dtype=_name(dtype), device=case.dev)
    other.cluster_centers_ = case.C + 1
    with pytest.raises(ValueError, match="centres"):
        other.load_pq_index(tmp_path / "pq")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_name)
def test_trained_index_searches(dtype):
    """The whole path with trained codebooks: a row's own query finds it first."""
    case = _cases.get((64, 16, dtype)) or Case(64, 16, dtype)
    _cases[(64, 16, dtype)] = case
    km = mikmeans.KMeans(K, dtype=_name(case.dtype), device=case.dev, seed=3)
    km.cluster_centers_ = case.C.clone()
    a = km.build_pq_index(case.X, 16, train_rows=1024, pq_max_iter=4)
    b = km.build_pq_index(case.X, 16, train_rows=1024, pq_max_iter=4, block_rows=700)
    assert torch.equal(a.codebooks, b.codebooks) and torch.equal(a._index.codes, b._index.codes)
    rows, _ = a.search(case.X[100:140], 1, nprobe=2)
    assert int((rows[:, 0] == torch.arange(100, 140, device=case.dev)).sum()) >= 30


def test_errors(case):
    dtype, M, F = case.dtype, case.M, case.F
    km = mikmeans.KMeans(K, dtype=_name(dtype), device=case.dev)
    km.cluster_centers_ = case.C.clone()
    with pytest.raises(ValueError, match=r"\(8, 16, 32, 64\)"):
        km.build_pq_index(case.X, 12)
    if F % 64:
        with pytest.raises(ValueError, match=r"\(8, 16, 32, 64\)"):
            km.build_pq_index(case.X, 64)                                       # F % M != 0
    with pytest.raises(ValueError, match="at least 256"):
        km.build_pq_index(case.X[:200], M)
    ix = mikmeans.PQIndex(km, case.index)
    for m in (0, 33):
        with pytest.raises(ValueError, match="1 <= m <= 32"):
            ix.search(case.Q, m)
    for nprobe in (0, K + 1):
        with pytest.raises(ValueError, match="nprobe"):
            ix.search(case.Q, 1, nprobe=nprobe)
    wide = torch.zeros((3, F + 16), dtype=dtype, device=case.dev)
    with pytest.raises(ValueError, match="features"):
        ops.pq_search(case.index, wide, case.C, 1, 1)
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    with pytest.raises(ValueError, match="features"):
        ops.pq_search(case.index, case.Q.to(other), case.C, 1, 1)
