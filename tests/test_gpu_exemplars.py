"""The per-cluster exemplar kernel (csrc/exemplars.hip) and cluster_exemplars on the GPU.

The oracle is the integer mirror ``ops.cpu.exemplar_table`` on the same (idx, d2): the native
table must equal it word for word in both of the kernel's forms and by the launcher's rule; end
to end the lists are the mirror's on ``ops.topk(X, C, 1)``'s output and agree with float64."""
import functools

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref
from tests.test_exemplars import assert_lists, brute_force

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
LDS_MAX_WORDS = 20480
INF, NAN = float("inf"), float("nan")

# (n, K, m, kind): one row; a ragged wave either side of 64; the longest lists with distances
# from four values only (every order decided by the row); K * m just under and just over what the
# LDS form holds (20480 words); several workgroups with labels outside the table and NaN / inf /
# -0.0 distances
SHAPES = [(1, 3, 2, "random"), (63, 3, 1, "random"), (65, 3, 4, "random"), (5000, 7, 32, "ties"),
          (5000, 7, 64, "ties"), (40_000, 1024, 16, "random"), (40_000, 1300, 16, "random"),
          (100_000, 37, 5, "hard")]


@functools.lru_cache(maxsize=None)
def _synthetic(n, K, kind):
    """(idx, d2) on the host as a top-1 result."""
    g = torch.Generator().manual_seed(n + 7 * K)
    k = torch.randint(0, K, (n,), generator=g).to(torch.int32)
    if kind == "ties":
        d = torch.tensor([0.0, 1.0, 2.0, 4.0])[torch.randint(0, 4, (n,), generator=g)]
    else:
        d = torch.rand(n, generator=g) * 100.0
    if kind == "hard":
        d[3::11] = -0.0
        d[4::13] = 0.0
        d[5::37] = NAN
        d[6::41] = INF
        d[7::43] = -INF
        d[10::47] = -1.5                                                  # (clamped to +0)
        k[8::29] = -1
        k[9::31] = K
        k[12::53] = 2**31 - 1
    return k.view(n, 1).contiguous(), d.view(n, 1).contiguous()


def _native_table(idx, d2, K, m, path=-1, row0=0, farthest=False, table=None):
    t = ops.exemplar_new(K, m, DEV) if table is None else table
    return ops.exemplar_accumulate(t, idx, d2, row0=row0, farthest=farthest, path=path)


def _all_paths(idx, d2, K, m, farthest):
    """The table by the launcher's rule; the forced global and LDS-private forms must equal it."""
    T = _native_table(idx, d2, K, m, farthest=farthest)
    assert torch.equal(_native_table(idx, d2, K, m, path=0, farthest=farthest), T)
    if K * m <= LDS_MAX_WORDS:
        assert torch.equal(_native_table(idx, d2, K, m, path=1, farthest=farthest), T)
    else:
        with pytest.raises(RuntimeError):                                 # the LDS form cannot hold the table
            _native_table(idx, d2, K, m, path=1, farthest=farthest)
    return T


def test_constants(native):
    assert native.EXEMPLAR_MAX == ops.EXEMPLAR_MAX == 64 and native.EXEMPLAR_LDS_MAX_WORDS == LDS_MAX_WORDS
    # the launcher's rule (csrc/kernels.h): the LDS form for K * m^2 <= 16384 from 8192 rows on
    assert native.EXEMPLAR_LDS_RULE_KMM == 16384 and native.EXEMPLAR_LDS_MIN_ROWS == 8192
    for n, K, m, _ in SHAPES + [(8191, 16, 32, ""), (8192, 16, 32, ""), (1 << 22, 1024, 4, ""), (1 << 22, 1024, 5, "")]:
        assert native.exemplar_uses_lds(n, K, m) == (K * m * m <= 16384 and n >= 8192), (n, K, m)
    idx, d2 = _synthetic(63, 3, "random")
    with pytest.raises(ValueError):
        _native_table(idx.to(DEV), d2.to(DEV), 3, 65)
    with pytest.raises(ValueError):
        _native_table(idx.to(DEV), d2.to(DEV), 3, 4, row0=(1 << 32) - 62)
    # the last row index a key holds (63 rows in lists of 64: every row is listed)
    T = _native_table(idx.to(DEV), d2.to(DEV), 3, 64, row0=(1 << 32) - 63)
    assert torch.equal(T.cpu(), ref.exemplar_table(idx, d2, 3, 64, row0=(1 << 32) - 63))
    assert int(ops.exemplar_decode(T)[0].max()) == (1 << 32) - 1


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("n,K,m,kind", SHAPES)
def test_kernel_is_the_mirror(native, n, K, m, kind, farthest):
    idx, d2 = _synthetic(n, K, kind)
    T = _all_paths(idx.to(DEV), d2.to(DEV), K, m, farthest)
    M = ref.exemplar_table(idx, d2, K, m, farthest=farthest)
    assert torch.equal(T.cpu(), M), (T.cpu() != M).nonzero()[:8]
    if n <= 5000 or kind == "hard":
        assert_lists(*ops.exemplar_decode(T, farthest=farthest), *brute_force(idx, d2, K, m, farthest=farthest))


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("path", [0, 1])
def test_contention_on_one_list(native, path, farthest):
    """Every row in cluster 0 and every row nearer (farther) than all before it: no read of the
    last slot turns an insert away, all of them meet on one list."""
    n, m = 60_000, 32
    idx = torch.zeros((n, 1), dtype=torch.int32)
    for d in (torch.arange(n, 0, -1), torch.arange(1, n + 1)):           # strictly decreasing, increasing
        d2 = d.to(torch.float32).view(n, 1)
        T = _native_table(idx.to(DEV), d2.to(DEV), 2, m, path=path, farthest=farthest)
        assert torch.equal(T.cpu(), ref.exemplar_table(idx, d2, 2, m, farthest=farthest))
        rows = ops.exemplar_decode(T, farthest=farthest)[0][0].cpu()
        from_the_end = bool(d2[0, 0] > d2[1, 0]) != farthest              # the listed rows are the last m
        by_row = torch.arange(n - 1, n - 1 - m, -1) if from_the_end else torch.arange(m)
        assert torch.equal(rows, by_row) and bool((T[1] == -1).all())


@pytest.mark.parametrize("farthest", [False, True])
def test_row_blocks_accumulate(native, farthest):
    n, K, m = 100_000, 37, 5
    idx, d2 = _synthetic(n, K, "hard")
    idx, d2 = idx[:20_000].to(DEV), d2[:20_000].to(DEV)
    one = _native_table(idx, d2, K, m, farthest=farthest)
    for path in (0, 1):
        acc = ops.exemplar_new(K, m, DEV)
        for s in reversed(range(0, 20_000, 777)):
            _native_table(idx[s : s + 777], d2[s : s + 777], K, m, path=path, row0=s, farthest=farthest, table=acc)
        assert torch.equal(acc, one)
    # column 0 is read through the row stride of a top-2 result
    wide = torch.stack([idx[:, 0], idx[:, 0] + 1], 1).contiguous(), torch.stack([d2[:, 0], d2[:, 0] + 1], 1).contiguous()
    for path in (0, 1):
        assert torch.equal(_native_table(*wide, K, m, path=path, farthest=farthest), one)


# ---- end to end ------------------------------------------------------------------------------
E2E = [(3000, 128, 1024, 4), (513, 30, 37, 8), (1200, 1000, 130, 3)]


def _points(n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, n, d, k):
    X = _points(n, d, dtype, seed=n + k)
    C = _points(k, d, torch.float32, seed=k + 3)
    idx, d2 = ops.topk(X.to(DEV), C.to(DEV), 1)
    return X, C, idx.cpu(), d2.cpu()


def _model(cls, C, dtype, **kw):
    km = cls(C.shape[0], dtype=dtype, **kw)
    km.cluster_centers_ = C.to(DEV)
    return km


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", E2E)
def test_estimator_is_the_mirror_on_top1(native, dtype, n, d, k, m, farthest):
    X, C, idx, d2 = _case(dtype, n, d, k)
    km = _model(mikmeans.KMeans, C, "bfloat16" if dtype == torch.bfloat16 else "float32")
    Xd = X.to(DEV)
    rows, sq = km.cluster_exemplars(Xd, m, farthest=farthest, squared=True)
    assert rows.is_cuda and sq.is_cuda
    exp = ops.exemplar_decode(ref.exemplar_table(idx, d2, k, m, farthest=farthest), farthest=farthest)
    assert_lists(rows, sq, exp[0].numpy(), exp[1].numpy())
    rows2, dist = km.cluster_exemplars(Xd, m, farthest=farthest)
    assert torch.equal(rows2, rows) and torch.equal(dist.view(torch.int32), sq.sqrt().view(torch.int32))
    # row blocks, host rows in blocks, numpy in / numpy out
    b = km.cluster_exemplars(Xd, m, farthest=farthest, squared=True, block_rows=777)
    assert_lists(b[0], b[1], exp[0].numpy(), exp[1].numpy())
    h = km.cluster_exemplars(X, m, farthest=farthest, squared=True, block_rows=777)
    assert h[0].is_cuda
    assert_lists(h[0], h[1], exp[0].numpy(), exp[1].numpy())
    nr, nd = km.cluster_exemplars(X.float().numpy(), m, farthest=farthest, squared=True)
    assert isinstance(nr, np.ndarray) and isinstance(nd, np.ndarray)
    assert_lists(nr, nd, exp[0].numpy(), exp[1].numpy())
    # the functional form
    fr, fd = mikmeans.cluster_exemplars(Xd, C.to(DEV), m, dtype="bfloat16" if dtype == torch.bfloat16 else "float32",
                                        farthest=farthest)
    assert torch.equal(fr, rows) and torch.equal(fd.view(torch.int32), dist.view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", E2E)
def test_farthest_is_the_reports_radius(native, dtype, n, d, k, m):
    X, C, _, _ = _case(dtype, n, d, k)
    km = _model(mikmeans.KMeans, C, "bfloat16" if dtype == torch.bfloat16 else "float32")
    rep = km.cluster_report(X.to(DEV))
    rows, sq = km.cluster_exemplars(X.to(DEV), m, farthest=True, squared=True)
    full = rep.counts > 0
    assert torch.equal(sq[full, 0].view(torch.int32).long(), rep.table[full, 17])
    assert torch.equal((rows >= 0).sum(1), rep.counts.clamp_max(m))
    near, _ = km.cluster_exemplars(X.to(DEV), m)
    assert torch.equal((near >= 0).sum(1), rep.counts.clamp_max(m))


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", E2E)
def test_exemplars_against_float64(native, dtype, n, d, k, m, farthest):
    """Independent of every kernel: float64 distances to the quantised centres, with
    test_gpu_topk.py::test_topk_against_float64's per-row tolerance.  Each listed row's float64
    distance to its centre is at most the float64 m-th smallest (at least the m-th largest) among
    the rows float64 assigns to that cluster, within 2 tol (no bound from a cluster to which
    float64 assigns fewer than m rows); the row is one float64 could assign there (within 2 tol
    of its nearest centre); and the returned distance is within tol of float64."""
    X, C, _, _ = _case(dtype, n, d, k)
    km = _model(mikmeans.KMeans, C, "bfloat16" if dtype == torch.bfloat16 else "float32")
    rows, dist = km.cluster_exemplars(X.to(DEV), m, farthest=farthest)
    rows, dist = rows.cpu(), dist.cpu().double()
    Cq = ref.quantize_centers(C, dtype).double()
    exp = torch.cdist(X.double(), Cq)
    tol = ((3e-5 if dtype == torch.float32 else 1e-4) * (X.double().norm(dim=1) + Cq.norm(dim=1).max()) + 1e-3)
    best, lab = exp.min(dim=1)
    listed = 0
    for c in range(k):
        r = rows[c][rows[c] >= 0]
        if not r.numel():
            continue
        listed += r.numel()
        true = exp[r, c]
        own = exp[lab == c, c]
        assert bool(((dist[c, : r.numel()] - true).abs() <= tol[r]).all()), c
        assert bool((true <= best[r] + 2 * tol[r]).all()), c
        if own.numel() >= m:
            if farthest:
                bound = own.sort(descending=True).values[m - 1]
                assert bool((true >= bound - 2 * tol[r]).all()), (c, float((bound - true).max()))
            else:
                bound = own.sort().values[m - 1]
                assert bool((true <= bound + 2 * tol[r]).all()), (c, float((true - bound).max()))
        o = dist[c, : r.numel()]
        assert bool((o[1:] <= o[:-1]).all() if farthest else (o[1:] >= o[:-1]).all())
    assert listed > 0


def test_cosine_and_minibatch_models(native):
    X = _points(3000, 40, torch.float32, seed=5).to(DEV)
    km = mikmeans.KMeans(9, metric="cosine", seed=0, max_iter=5).fit(X)
    rows, sq = km.cluster_exemplars(X, 6, farthest=True, squared=True)
    idx, d2 = km.predict_topk(X, 1, squared=True)
    assert_lists(rows, sq, *brute_force(idx, d2, 9, 6, farthest=True))
    assert float(sq.max()) <= 4.0 + 1e-5
    h = km.cluster_exemplars(X.cpu(), 6, farthest=True, squared=True)            # host rows
    assert torch.equal(h[0], rows) and torch.equal(h[1], sq)
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, seed=0).fit(X)
    rows, sq = mb.cluster_exemplars(X, 3, squared=True)
    idx, d2 = ops.topk(X, mb.cluster_centers_, 1)
    assert_lists(rows, sq, *brute_force(idx, d2, 8, 3))
