"""The per-cluster quality kernel (csrc/quality.hip) and cluster_report on the GPU.

The oracle is the integer mirror ``ops.cpu.quality_table`` on the same top-2 output: the count,
sum-of-squares digit, non-finite and maximum words must be equal word for word; the
sum-of-distances digits and the silhouette word may differ by the device's float64 sqrt / divide
rounding (a unit in the last place per row), within the CPU test's bounds."""
import functools

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.data import blobs as B
from mikmeans.ops import cpu as ref
from tests.test_quality import QW, check_against_numpy, hard_inputs, words_int

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]

# (n, D, K): one row; a ragged wave either side of 64; several workgroups with K no multiple of
# anything; mostly empty clusters; wide rows; K = 1 (m = 1) and K = 2.  Then the launcher's rule
# (csrc/kernels.h): batches of QUALITY_LDS_MIN_ROWS rows and K <= QUALITY_LDS_MAX_K take the
# LDS-private kernel -- one row under and exactly at the row threshold, the largest K it holds
# (all 160 KiB of LDS) and the first K past it.  Last, row blocks just past a single pass of
# either grid, so the grid-stride loops wrap for the first 77 threads: the LDS form's
# (256 x 1024 rows) and the global form's (2048 x 256 rows; every case also runs with each
# form forced, so that one covers the global kernel's loop and wraps the LDS one twice).
PASS_ROWS, LDS_PASS_ROWS, LDS_MAX_K, LDS_MIN_ROWS = 2048 * 256, 256 * 1024, 1137, 8192
SHAPES = [(1, 128, 1024), (63, 16, 3), (65, 16, 3), (513, 30, 37), (3000, 128, 1024), (1200, 1000, 130),
          (50, 16, 1), (50, 16, 2), (LDS_MIN_ROWS - 1, 16, 37), (LDS_MIN_ROWS, 16, 37), (9000, 16, LDS_MAX_K),
          (9000, 16, LDS_MAX_K + 1), (LDS_PASS_ROWS + 77, 16, 3), (PASS_ROWS + 77, 16, 3)]


def _points(n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, n, d, k):
    X = _points(n, d, dtype, seed=n + k).to(DEV)
    C = _points(k, d, torch.float32, seed=k + 3).to(DEV)
    idx, d2 = ops.topk(X, C, min(2, k))
    return X, C, idx, d2


def _native_table(idx, d2, K, path=-1):
    t = torch.zeros((K, QW), dtype=torch.int64, device=DEV)
    return ops.quality_accumulate(t, idx, d2, path=path)


def _all_paths(idx, d2, K):
    """The table by the launcher's rule; the forced global and LDS-private forms must equal it."""
    T = _native_table(idx, d2, K)
    assert torch.equal(_native_table(idx, d2, K, path=0), T)
    if K <= LDS_MAX_K:
        assert torch.equal(_native_table(idx, d2, K, path=1), T)
    return T


def assert_matches_mirror(T, idx, d2, K):
    """Native table == mirror: exact in the integer-only words, within the rounding bounds in
    the two that go through a float64 sqrt / divide."""
    M = ref.quality_table(idx.cpu(), d2.cpu(), K)
    T = T.cpu()
    exact = [*range(0, 8), 15, 17, *range(18, QW)]
    assert torch.equal(T[:, exact], M[:, exact]), (T[:, exact] != M[:, exact]).nonzero()[:8]
    for c in range(K):
        nk = int(M[c, 7])
        sa = words_int(M[c], 8)
        assert abs(words_int(T[c], 8) - sa) / 2.0 ** 64 <= 1e-12 * (sa / 2.0 ** 64) + nk * 2.0 ** -60, c
        assert abs(int(T[c, 16]) - int(M[c, 16])) / 2.0 ** 31 <= nk * 2.0 ** -30, c


def test_launch_geometry(native):
    assert native.QUALITY_PASS_ROWS == PASS_ROWS and native.QUALITY_WORDS == QW
    assert native.QUALITY_LDS_PASS_ROWS == LDS_PASS_ROWS and native.QUALITY_LDS_MAX_K == LDS_MAX_K
    assert native.QUALITY_LDS_MIN_ROWS == LDS_MIN_ROWS
    for n, _, k in SHAPES:
        assert native.quality_uses_lds(n, k) == (n >= LDS_MIN_ROWS and k <= LDS_MAX_K)
    idx, d2, _ = hard_inputs()["mixed"]
    with pytest.raises(RuntimeError):                                # the LDS form cannot hold that many labels
        _native_table(idx.to(DEV), d2.to(DEV), LDS_MAX_K + 1, path=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k", SHAPES)
def test_kernel_is_the_mirror(native, dtype, n, d, k):
    _, _, idx, d2 = _case(dtype, n, d, k)
    assert idx.shape == (n, min(2, k))
    T = _all_paths(idx, d2, k)
    assert_matches_mirror(T, idx, d2, k)
    assert int(T[:, 7].sum()) + int(T[:, 15].sum()) == n


@pytest.mark.parametrize("name", sorted(hard_inputs()))
def test_kernel_hard_inputs(native, name):
    idx, d2, K = hard_inputs()[name]
    T = _all_paths(idx.to(DEV), d2.to(DEV), K)
    assert_matches_mirror(T, idx, d2, K)
    check_against_numpy(T, idx, d2, K)


def test_labels_outside_the_table_are_skipped(native):
    idx, d2, K = hard_inputs()["nonfinite"]
    idx = idx.clone()
    idx[::7, 0] = -1
    idx[3::7, 0] = K
    T = _all_paths(idx.to(DEV), d2.to(DEV), K)
    assert_matches_mirror(T, idx, d2, K)
    assert int(T[:, 7].sum()) + int(T[:, 15].sum()) == int(((idx[:, 0] >= 0) & (idx[:, 0] < K)).sum())


def test_order_freedom(native):
    X, C, idx, d2 = _case(torch.bfloat16, 3000, 128, 1024)
    T = _native_table(idx, d2, 1024)
    for path in (0, 0, 1, 1):
        assert torch.equal(_native_table(idx, d2, 1024, path=path), T)
    p = torch.randperm(3000, generator=torch.Generator().manual_seed(1)).to(DEV)
    assert torch.equal(_native_table(idx[p].contiguous(), d2[p].contiguous(), 1024), T)
    for block in (None, 1000, 1):
        rep, Tb = ops.cluster_quality(X, C, block_rows=block)
        assert torch.equal(Tb, T), block
    assert rep["n_samples"] == 3000 and int(rep["counts"].sum()) == 3000


@pytest.mark.parametrize("dtype", DTYPES)
def test_end_to_end_blobs(native, dtype):
    """Well-separated blobs under their true centres: the generator's labels, and every
    cluster's mean distance within test_gpu_topk.py::test_topk_against_float64's per-row
    tolerance (its maximum over the cluster's rows) of float64 cdist."""
    n, d, k = 6000, 64, 8
    X, y = B.make_blobs(n, d, k, seed=5, dtype=dtype, return_labels=True)
    C = B.blob_centers(k, d, 10.0, 5)
    Cq = ref.quantize_centers(C, dtype).double()
    exp = torch.cdist(X.double(), Cq)
    tol = (3e-5 if dtype == torch.float32 else 1e-4) * (X.double().norm(dim=1) + Cq.norm(dim=1).max()) + 1e-3
    two = exp.sort(dim=1)
    assert bool((two.values[:, 1] - two.values[:, 0] > 2 * tol).all())        # no label can differ
    assert torch.equal(two.indices[:, 0], y.long())
    rep, T = ops.cluster_quality(X.to(DEV), C.to(DEV))
    assert torch.equal(rep["counts"], torch.bincount(y.long(), minlength=k))
    for c in range(k):
        rows = y == c
        err = abs(float(rep["mean_distance"][c]) - float(two.values[rows, 0].mean()))
        assert err <= float(tol[rows].max()), (c, err)
        assert abs(float(rep["radius"][c]) - float(two.values[rows, 0].max())) <= float(tol[rows].max())
    s = float((1 - two.values[:, 0] / two.values[:, 1]).mean())
    assert rep["silhouette"] == pytest.approx(s, abs=1e-3) and 0 < rep["davies_bouldin"] < 1


def _model(cls, C, dtype, **kw):
    km = cls(C.shape[0], dtype=dtype, **kw)
    km.cluster_centers_ = C.to(DEV)
    return km


def test_estimator_cluster_report(native):
    X = _points(5000, 64, torch.bfloat16, seed=1)
    C = _points(48, 64, torch.float32, seed=2)
    km = _model(mikmeans.KMeans, C, "bfloat16")
    Xd = X.to(DEV)
    _, T = ops.cluster_quality(Xd, C.to(DEV))
    rep = km.cluster_report(Xd)
    assert rep.table.is_cuda and rep.counts.is_cuda and torch.equal(rep.table, T)
    assert rep.n_samples == 5000 and torch.equal(rep.counts.cpu(), torch.bincount(
        ops.topk(Xd, C.to(DEV), 1)[0][:, 0].long().cpu(), minlength=48))
    # host rows bound for the GPU model: one shot, in blocks, and numpy in / numpy out
    assert torch.equal(km.cluster_report(X).table, T)
    blocked = km.cluster_report(X, block_rows=777)
    assert torch.equal(blocked.table, T) and blocked.to_dict() == rep.to_dict()
    nrep = km.cluster_report(X.float().numpy(), block_rows=1300)
    assert isinstance(nrep.table, np.ndarray) and np.array_equal(nrep.table, T.cpu().numpy())
    frep = mikmeans.cluster_report(Xd, C.to(DEV), dtype="bfloat16")
    assert torch.equal(frep.table, T) and frep.davies_bouldin == rep.davies_bouldin
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, dtype="bfloat16", seed=0).fit(Xd)
    mrep = mb.cluster_report(Xd)
    assert torch.equal(mrep.table, ops.cluster_quality(Xd, mb.cluster_centers_)[1]) and mrep.n_samples == 5000


def test_cosine_model(native):
    X = _points(3000, 40, torch.float32, seed=5)
    km = mikmeans.KMeans(9, metric="cosine", seed=0, max_iter=5).fit(X.to(DEV))
    rep = km.cluster_report(X.to(DEV))
    idx, dist = km.predict_topk(X.to(DEV), 2, squared=True)
    assert torch.equal(rep.table, _native_table(idx, dist, 9))
    assert float(rep.radius.max()) <= 2.0 + 1e-5 and rep.n_samples == 3000
    assert torch.equal(km.cluster_report(X).table, rep.table)                # host rows
