"""The radix-select kernels (csrc/quantiles.hip) and cluster_quantiles on the GPU.

The oracle is the integer mirror ``ops.cpu.quantile_hist`` / ``quantile_select`` on the same
(idx, d2): after every pass the native histogram must equal it word for word in each of the
kernel's forms (global, LDS-private, banded LDS), by the launcher's rule and for any
wave-aggregation depth, and the select's
prefixes, ranks and counts must be the mirror's; end to end the values are the mirror's on
``ops.topk(X, C, 1)``'s output and agree with float64."""
import functools

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref
from tests.test_gpu_exemplars import _synthetic
from tests.test_quantiles import QS, assert_values, brute_force

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
LDS_MAX_LISTS = 160
BAND_LIMIT = 64
BAND_MAX_PASS0, BAND_MAX, BAND_MIN_ROWS = 26, 8, 1 << 18    # the banded form's rule (profiles/r7_03_quantiles.md)
Q8 = (0.0, 0.05, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0)

# (n, K, kind, q): one row; a ragged wave either side of 64; ties with all eight quantiles; K just
# at what the LDS form holds in pass 0 (with one quantile the later passes fit too) and just past
# it; several workgroups with labels outside the table and NaN / inf / -0.0 / negative distances
CASES = [(1, 3, "random", QS), (63, 3, "random", QS), (65, 3, "random", QS), (5000, 7, "ties", Q8),
         (40_000, 160, "random", QS), (40_000, 160, "random", (0.5,)), (40_000, 161, "random", QS),
         (100_000, 37, "hard", QS)]


def _hist(idx, d2, K, prefix, p, **kw):
    return ops.quantile_hist(idx, d2, K, prefix, p, **kw)


def _all_forms(idx, d2, K, prefix, p, expect):
    """The pass's table by the launcher's rule; the forced global and LDS-private forms, without
    wave aggregation and with as many rounds as a wave has lanes, must all be ``expect``."""
    lists = K if p == 0 else K * prefix.shape[1]
    T = _hist(idx, d2, K, prefix, p)
    assert torch.equal(T.cpu(), expect), (p, (T.cpu() != expect).nonzero()[:8])
    for agg in (-1, 0, 64):
        assert torch.equal(_hist(idx, d2, K, prefix, p, path=0, agg=agg), T), (p, agg)
        if lists <= LDS_MAX_LISTS:
            assert torch.equal(_hist(idx, d2, K, prefix, p, path=1, agg=agg), T), (p, agg)
        if lists <= LDS_MAX_LISTS * BAND_LIMIT:                           # the banded form: ceil(lists / 160) bands
            assert torch.equal(_hist(idx, d2, K, prefix, p, path=2, agg=agg), T), (p, agg)
    if lists > LDS_MAX_LISTS:
        with pytest.raises(RuntimeError):                                 # one workgroup's LDS cannot hold the table
            _hist(idx, d2, K, prefix, p, path=1)
    return T


def _passes_match_mirror(idx, d2, K, qs):
    """All four passes on the device beside the mirror; returns the device (prefix, counts)."""
    di, dd = idx.to(DEV), d2.to(DEV)
    q = torch.tensor(qs, dtype=torch.float64)
    P, R, N = ops.quantile_state(K, len(qs))
    gP, gR, gN = ops.quantile_state(K, len(qs), DEV)
    for p in range(4):
        M = ref.quantile_hist(idx, d2, K, P, p)
        T = _all_forms(di, dd, K, gP, p, M)
        ops.quantile_select(T, q.to(DEV), gP, gR, gN, p)
        P, R, n = ref.quantile_select(M, q, P, R, p)
        N = n if p == 0 else N
        assert torch.equal(gP.cpu(), P) and torch.equal(gR.cpu(), R) and torch.equal(gN.cpu(), N), p
    return gP, gN


def test_constants(native):
    assert native.QUANTILE_MAX_Q == ops.QUANTILE_MAX_Q == 8 and native.QUANTILE_BINS == ops.QUANTILE_BINS == 256
    assert native.QUANTILE_LDS_MAX_LISTS == LDS_MAX_LISTS == 160 * 1024 // (256 * 4)
    # the launcher's rule and the wave-aggregation depths of the two forms, as measured
    # (csrc/kernels.h, profiles/r7_03_quantiles.md)
    assert native.QUANTILE_LDS_MIN_ROWS == 8192
    assert native.QUANTILE_AGG_ROUNDS == 2 and native.QUANTILE_LDS_AGG_ROUNDS == 0
    for n, lists in [(1, 3), (8191, 8), (8192, 8), (40_000, 160), (40_000, 161), (1 << 22, 1), (1 << 22, 160),
                     (1 << 22, 1024), ((1 << 32) - 1, 8), (1 << 32, 8)]:
        assert native.quantile_uses_lds(n, lists) == (lists <= 160 and 8192 <= n < 1 << 32), (n, lists)
    # past one workgroup's LDS: the banded form, in pass 0 up to 26 bands of 160 lists and in pass 1
    # up to 8, from BAND_MIN_ROWS rows on; passes 2 and 3 stay with the global form
    assert native.QUANTILE_BAND_LIMIT == BAND_LIMIT and native.QUANTILE_BAND_MAX_PASS0 == BAND_MAX_PASS0
    assert (native.QUANTILE_BAND_MAX, native.QUANTILE_BAND_MIN_ROWS) == (BAND_MAX, BAND_MIN_ROWS)
    for n, lists in [(8192, 160), (1 << 22, 160), (BAND_MIN_ROWS - 1, 161), (BAND_MIN_ROWS, 161), (1 << 22, 161),
                     (1 << 22, 160 * BAND_MAX), (1 << 22, 160 * BAND_MAX + 1), (1 << 22, 160 * BAND_MAX_PASS0),
                     (1 << 22, 160 * BAND_MAX_PASS0 + 1), (1 << 32, 161), (100, 3), (1 << 22, 32768)]:
        for p in range(4):
            most = (BAND_MAX_PASS0, BAND_MAX, 0, 0)[p]
            exp = 1 if lists <= 160 and 8192 <= n < 1 << 32 else (
                2 if 160 < lists <= 160 * most and BAND_MIN_ROWS <= n < 1 << 32 else 0)
            assert native.quantile_path(n, lists, p) == exp, (n, lists, p)
    idx, d2 = (t.to(DEV) for t in _synthetic(63, 3, "random"))
    with pytest.raises(RuntimeError):                                     # more bands than the banded form holds
        native.quantile_hist(idx, d2, torch.zeros((160 * BAND_LIMIT + 1, 256), dtype=torch.int64, device=DEV), None, 0, 2)
    with pytest.raises(ValueError):
        ops.quantile_state(3, 9, DEV)
    with pytest.raises(RuntimeError):                                     # nine quantiles
        native.quantile_hist(idx, d2, torch.zeros((3, 9, 256), dtype=torch.int64, device=DEV),
                             torch.zeros((3, 9), dtype=torch.int32, device=DEV), 1)
    with pytest.raises(RuntimeError):                                     # passes 1..3 need the prefixes
        native.quantile_hist(idx, d2, torch.zeros((3, 2, 256), dtype=torch.int64, device=DEV), None, 1)
    with pytest.raises(RuntimeError):
        native.quantile_hist(idx, d2, torch.zeros((3, 256), dtype=torch.int64, device=DEV), None, 4)


@pytest.mark.parametrize("n,K,kind,qs", CASES)
def test_kernel_is_the_mirror(native, n, K, kind, qs):
    idx, d2 = _synthetic(n, K, kind)
    P, N = _passes_match_mirror(idx, d2, K, qs)
    values = torch.where((N > 0)[:, None], P.view(torch.float32), float("nan"))
    assert_values(values, N, *brute_force(idx, d2, K, qs))
    v, c = ops.quantile_passes([(idx.to(DEV), d2.to(DEV))], K, qs, DEV)
    assert torch.equal(v.view(torch.int32), values.view(torch.int32)) and torch.equal(c, N)


def test_contention_on_one_list(native):
    """Every row in cluster 0: with one identical distance every lane of every wave meets on one
    bin in every pass; with strictly increasing distances the lanes of a wave share the high
    digits and spread over the low ones."""
    n = 60_000
    idx = torch.zeros((n, 1), dtype=torch.int32)
    for d2 in (torch.full((n, 1), 3.5), torch.arange(1, n + 1).to(torch.float32).view(n, 1)):
        P, N = _passes_match_mirror(idx, d2, 2, QS)
        assert N.tolist() == [n, 0]
        exp = [float(d2[min(max(int(np.ceil(np.float64(q) * n)) - 1, 0), n - 1), 0]) for q in QS]
        assert P[0].view(torch.float32).tolist() == exp


def test_row_blocks_accumulate(native):
    K, qs = 37, (0.1, 0.5, 0.9, 1.0)                                      # (K * Q = 148 lists: every form in every pass)
    idx, d2 = _synthetic(100_000, K, "hard")
    idx, d2 = idx[:20_000], d2[:20_000]
    di, dd = idx.to(DEV), d2.to(DEV)
    wide = torch.stack([di[:, 0], di[:, 0] + 1], 1).contiguous(), torch.stack([dd[:, 0], dd[:, 0] + 1], 1).contiguous()
    q = torch.tensor(qs, dtype=torch.float64, device=DEV)
    P, R, N = ops.quantile_state(K, len(qs), DEV)
    for p in range(4):
        one = _hist(di, dd, K, P, p)
        for path in (0, 1, 2):
            acc = None
            for s in reversed(range(0, 20_000, 777)):
                acc = _hist(di[s : s + 777], dd[s : s + 777], K, P, p, table=acc, path=path)
            assert torch.equal(acc, one), (p, path)
            # column 0 is read through the row stride of a top-2 result
            assert torch.equal(_hist(*wide, K, P, p, path=path), one), (p, path)
        ops.quantile_select(one, q, P, R, N, p)
    assert_values(torch.where((N > 0)[:, None], P.view(torch.float32), float("nan")), N, *brute_force(idx, d2, K, qs))


# ---- end to end ------------------------------------------------------------------------------
E2E = [(3000, 128, 1024), (513, 30, 37), (1200, 1000, 130)]


def _points(n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, n, d, k):
    X = _points(n, d, dtype, seed=n + k)
    C = _points(k, d, torch.float32, seed=k + 3)
    idx, d2 = ops.topk(X.to(DEV), C.to(DEV), 1)
    return X, C, idx.cpu(), d2.cpu()


def _name(dtype):
    return "bfloat16" if dtype == torch.bfloat16 else "float32"


def _model(cls, C, dtype, **kw):
    km = cls(C.shape[0], dtype=_name(dtype), **kw)
    km.cluster_centers_ = C.to(DEV)
    return km


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k", E2E)
def test_estimator_is_the_mirror_on_top1(native, dtype, n, d, k):
    X, C, idx, d2 = _case(dtype, n, d, k)
    km = _model(mikmeans.KMeans, C, dtype)
    Xd = X.to(DEV)
    sq, counts = km.cluster_quantiles(Xd, QS, squared=True)
    assert sq.is_cuda and counts.is_cuda
    ev, ec = ops.quantile_passes([(idx, d2)], k, QS)                       # the mirror
    assert_values(sq, counts, ev.numpy(), ec.numpy())
    assert_values(sq, counts, *brute_force(idx, d2, k, QS))
    dist, c2 = km.cluster_quantiles(Xd, QS)
    assert torch.equal(c2, counts) and torch.equal(dist.view(torch.int32), sq.sqrt().view(torch.int32))
    # row blocks, host rows in blocks, numpy in / numpy out
    b = km.cluster_quantiles(Xd, QS, squared=True, block_rows=777)
    assert_values(b[0], b[1], ev.numpy(), ec.numpy())
    h = km.cluster_quantiles(X, QS, squared=True, block_rows=777)
    assert h[0].is_cuda
    assert_values(h[0], h[1], ev.numpy(), ec.numpy())
    nv, nc = km.cluster_quantiles(X.float().numpy(), QS, squared=True)
    assert isinstance(nv, np.ndarray) and isinstance(nc, np.ndarray)
    assert_values(nv, nc, ev.numpy(), ec.numpy())
    # the functional form
    fv, fc = mikmeans.cluster_quantiles(Xd, C.to(DEV), QS, dtype=_name(dtype))
    assert torch.equal(fc, counts) and torch.equal(fv.view(torch.int32), dist.view(torch.int32))
    # q = 1 is the report's radius word, q = 0 the nearest exemplar, the counts the report's
    rep = km.cluster_report(Xd)
    full = rep.counts > 0
    assert torch.equal(counts, rep.counts)
    assert torch.equal(sq[full, -1].view(torch.int32).long(), rep.table[full, 17])
    near = km.cluster_exemplars(Xd, 1, squared=True)[1]
    assert torch.equal(sq[:, 0].view(torch.int32), near[:, 0].view(torch.int32))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k", E2E)
def test_quantiles_against_float64(native, dtype, n, d, k):
    """Independent of every kernel: for each non-empty cluster the rows the kernel assigned to it
    (predict_topk's first column), their float64 distances to the quantised centre sorted into
    e, and |value - e[r]| <= the largest per-row tolerance of test_gpu_topk.py among those rows:
    order statistics are 1-Lipschitz under a pointwise perturbation of the distances."""
    X, C, _, _ = _case(dtype, n, d, k)
    km = _model(mikmeans.KMeans, C, dtype)
    values, counts = km.cluster_quantiles(X.to(DEV), QS)
    values, counts = values.cpu().double(), counts.cpu()
    lab = km.predict_topk(X.to(DEV), 1)[0][:, 0].cpu().long()
    Cq = ref.quantize_centers(C, dtype).double()
    tol = ((3e-5 if dtype == torch.float32 else 1e-4) * (X.double().norm(dim=1) + Cq.norm(dim=1).max()) + 1e-3)
    checked = 0
    for c in range(k):
        rows = (lab == c).nonzero().flatten()
        assert int(counts[c]) == rows.numel()
        if not rows.numel():
            assert bool(values[c].isnan().all())
            continue
        e = (X[rows].double() - Cq[c]).norm(dim=1).sort().values
        nk = rows.numel()
        for j, q in enumerate(QS):
            r = min(max(int(np.ceil(np.float64(q) * np.float64(nk))) - 1, 0), nk - 1)
            err = abs(float(values[c, j]) - float(e[r]))
            assert err <= float(tol[rows].max()), (c, q, err, float(tol[rows].max()))
            checked += 1
    assert checked > 0


def test_cosine_and_minibatch_models(native):
    X = _points(3000, 40, torch.float32, seed=5).to(DEV)
    km = mikmeans.KMeans(9, metric="cosine", seed=0, max_iter=5).fit(X)
    sq, counts = km.cluster_quantiles(X, QS, squared=True)
    idx, d2 = km.predict_topk(X, 1, squared=True)
    assert_values(sq, counts, *brute_force(idx, d2, 9, QS))
    assert float(sq[counts > 0].max()) <= 4.0 + 1e-5 and int(counts.sum()) == 3000
    h = km.cluster_quantiles(X.cpu(), QS, squared=True)                        # host rows
    assert torch.equal(h[0].view(torch.int32), sq.view(torch.int32)) and torch.equal(h[1], counts)
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, seed=0).fit(X)
    sq, counts = mb.cluster_quantiles(X, QS, squared=True)
    idx, d2 = ops.topk(X, mb.cluster_centers_, 1)
    assert_values(sq, counts, *brute_force(idx, d2, 8, QS))
