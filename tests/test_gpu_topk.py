"""The fused top-m kernel (csrc/topk.hip) and predict_topk on the GPU.

The oracle is the transform kernel itself: ``ops.topk`` must return, bit for bit, the first m
columns of a stable sort of ``ops.transform(X, C, squared=True)`` -- the same squared distances
in the same order, equal ones by centre index -- and those distances must agree with float64."""
import functools

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.data import blobs as B
from mikmeans.ops import cpu as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]

# (n, D, K, m): one row / K a multiple of the tile; m = K < 16 with a ragged row block on either
# side of 16; D = 2; D -> DPAD 32 across the list sizes (8 | 9 | 32); several workgroups with
# 1, 8 and 32; a pad tile at the end and a guard that is sometimes false; ragged wide rows;
# DPAD 1024 with and without pad columns (m almost K); DPAD 768 with the long list; batches
# past the launcher's small-batch rule (n >= 32768 P), which run 4, 2 and 3 | 2 row blocks a wave
SHAPES = [(1, 128, 1024, 8), (15, 16, 3, 3), (17, 16, 3, 3), (1000, 2, 3, 1),
          (513, 30, 37, 8), (513, 30, 37, 9), (513, 30, 37, 32),
          (3000, 128, 1024, 1), (3000, 128, 1024, 8), (3000, 128, 1024, 32),
          (2000, 64, 4097, 32), (1500, 300, 77, 16), (1200, 1000, 130, 8), (1200, 1024, 33, 32),
          (777, 768, 100, 32), (131089, 64, 40, 8), (65553, 64, 40, 32), (98309, 256, 24, 8)]


def _points(n, d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, d, generator=g).to(dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, n, d, k):
    """Gaussian rows and centres with the transform kernel's sorted squared distances (computed
    once per shape: the m's of a shape and both checks share them)."""
    X = _points(n, d, dtype, seed=n + k)
    C = _points(k, d, torch.float32, seed=k + 3)
    v, i = torch.sort(ops.transform(X.to(DEV), C.to(DEV), squared=True), dim=1, stable=True)
    return X, C, v, i


def _assert_bitwise(got_idx, got_d2, v, i, m):
    assert got_idx.dtype == torch.int32 and got_d2.dtype == torch.float32
    assert got_idx.shape == got_d2.shape == (v.shape[0], m)
    assert torch.equal(got_d2, v[:, :m]), int((got_d2 != v[:, :m]).sum())
    assert torch.equal(got_idx.long(), i[:, :m]), int((got_idx.long() != i[:, :m]).sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", SHAPES)
def test_topk_is_the_sorted_transform_bitwise(native, dtype, n, d, k, m):
    X, C, v, i = _case(dtype, n, d, k)
    idx, d2 = ops.topk(X.to(DEV), C.to(DEV), m)
    _assert_bitwise(idx, d2, v, i, m)
    assert int(idx.min()) >= 0 and int(idx.max()) < k        # no pad centre


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", [(700, 24, 40, 8), (700, 24, 40, 32), (300, 300, 64, 16),
                                     (131089, 24, 40, 8), (65553, 24, 40, 32)])
def test_topk_exact_ties_go_to_the_lower_index(native, dtype, n, d, k, m):
    """Small integers (exact in bf16 and in the f32 accumulation) with every centre present at
    k and k + K/2 and one value four times: equal distances in index order."""
    g = torch.Generator().manual_seed(k + m)
    base = torch.randint(-3, 4, (k // 2, d), generator=g).float()
    base[k // 2 - 1] = base[0]
    C = torch.cat([base, base])
    X = torch.randint(-3, 4, (n, d), generator=g).to(dtype)
    v, i = torch.sort(ops.transform(X.to(DEV), C.to(DEV), squared=True), dim=1, stable=True)
    idx, d2 = ops.topk(X.to(DEV), C.to(DEV), m)
    _assert_bitwise(idx, d2, v, i, m)
    tie = d2[:, 1:] == d2[:, :-1]
    assert bool((idx[:, 1:][tie] > idx[:, :-1][tie]).all())
    assert float(tie.any(dim=1).float().mean()) >= 0.5       # (every row: its nearest centre is a duplicate)
    Xd, Cd = X.double().to(DEV), C.double().to(DEV)          # (integers: every f64 operation is exact)
    exact = (Xd * Xd).sum(1)[:, None] + (Cd * Cd).sum(1)[None, :] - 2 * (Xd @ Cd.T)
    assert torch.equal(d2.double(), exact.gather(1, idx.long()))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,k,m", SHAPES)
def test_topk_against_float64(native, dtype, n, d, k, m):
    X, C, _, _ = _case(dtype, n, d, k)
    idx, d2 = ops.topk(X.to(DEV), C.to(DEV), m)
    Cq = ref.quantize_centers(C, dtype).double()
    exp = torch.cdist(X.double(), Cq)
    tol = (3e-5 if dtype == torch.float32 else 1e-4) * (X.double().norm(dim=1, keepdim=True) + Cq.norm(dim=1).max()) \
        + 1e-3
    best = exp.sort(dim=1).values[:, :m]
    err = (d2.cpu().double().sqrt() - best).abs()
    assert bool((err <= tol).all()), float((err - tol).max())
    true = exp.gather(1, idx.cpu().long())
    assert bool((true <= best[:, -1:] + 2 * tol).all()), float((true - best[:, -1:] - 2 * tol).max())


def test_top1_is_predict(native):
    X = B.make_blobs(30_000, 96, 12, seed=2, dtype=torch.bfloat16, device=DEV)
    km = mikmeans.KMeans(12, dtype="bfloat16", seed=0, max_iter=10).fit(X)
    idx, dist = km.predict_topk(X, 1)
    top2 = km.transform(X).topk(2, largest=False).values
    clear = (top2[:, 1] - top2[:, 0]) > 1e-3
    assert float(clear.float().mean()) >= 0.9                # (1.0 on the CPU reference)
    assert torch.equal(idx[:, 0][clear], km.predict(X)[clear])
    assert torch.equal(dist[:, 0], top2[:, 0])


def _model(cls, C, dtype, **kw):
    km = cls(C.shape[0], dtype=dtype, **kw)
    km.cluster_centers_ = C.to(DEV)
    return km


def test_estimator_predict_topk(native):
    X = _points(5000, 64, torch.bfloat16, seed=1)
    C = _points(48, 64, torch.float32, seed=2)
    km = _model(mikmeans.KMeans, C, "bfloat16")
    Xd = X.to(DEV)
    oi, od = ops.topk(Xd, C.to(DEV), 5)
    idx, d2 = km.predict_topk(Xd, 5, squared=True)
    assert torch.equal(idx, oi) and torch.equal(d2, od)
    idx, dist = km.predict_topk(Xd, 5)
    assert torch.equal(idx, oi) and torch.equal(dist, od.sqrt())
    # numpy in, numpy out; host rows in small blocks are the one-shot device call
    ni, nd = km.predict_topk(X.float().numpy(), 5, squared=True)
    assert isinstance(ni, np.ndarray) and isinstance(nd, np.ndarray)
    assert np.array_equal(ni, oi.cpu().numpy()) and np.array_equal(nd, od.cpu().numpy())
    bi, bd = km.predict_topk(X, 5, squared=True, block_rows=777)
    assert bi.device.type == "cuda" and torch.equal(bi, oi) and torch.equal(bd, od)
    # a list past the kernel's 32: the transform kernel's distances sorted in row blocks
    v, i = torch.sort(ops.transform(Xd, C.to(DEV), squared=True), dim=1, stable=True)
    idx, d2 = km.predict_topk(Xd, 40, squared=True)
    _assert_bitwise(idx, d2, v, i, 40)
    for bad in (0, 49):
        with pytest.raises(ValueError):
            km.predict_topk(Xd, bad)
    with pytest.raises(ValueError):
        ops.topk(Xd, C.to(DEV), 49)
    mb = mikmeans.MiniBatchKMeans(8, batch_size=512, max_iter=5, dtype="bfloat16", seed=0).fit(Xd)
    mi, md = mb.predict_topk(Xd, 3, squared=True)
    ei, ed = ops.topk(Xd, mb.cluster_centers_, 3)
    assert torch.equal(mi, ei) and torch.equal(md, ed)


def test_cosine_and_wide_models(native):
    X = _points(3000, 40, torch.float32, seed=5)
    km = mikmeans.KMeans(9, metric="cosine", seed=0, max_iter=5).fit(X.to(DEV))
    idx, dist = km.predict_topk(X.to(DEV), 4)
    torch.testing.assert_close(dist, km.transform(X.to(DEV)).gather(1, idx.long()))
    assert idx.dtype == torch.int32 and bool((dist[:, 1:] >= dist[:, :-1]).all())
    # D > 1024: no native kernel, the PyTorch path answers
    Xw = _points(600, 1100, torch.float32, seed=6)
    Cw = _points(5, 1100, torch.float32, seed=7)
    kw = _model(mikmeans.KMeans, Cw, "float32")
    idx, dist = kw.predict_topk(Xw.to(DEV), 3)
    assert idx.shape == dist.shape == (600, 3) and idx.is_cuda
    exp = torch.cdist(Xw.double(), Cw.double()).sort(dim=1)
    assert torch.equal(idx.cpu().long(), exp.indices[:, :3])
    torch.testing.assert_close(dist.cpu().double(), exp.values[:, :3], rtol=1e-4, atol=1e-3)
