"""predict_topk on the CPU: the PyTorch reference op, the estimators, the functional API, the
CLI's ``predict --top`` and ``/api/predict``'s ``"top"`` (the GPU kernel: test_gpu_topk.py)."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np_topk(X, C, m):
    """float64 squared distances, stable argsort (ties to the lower centre index)."""
    d = ((X[:, None, :].astype(np.float64) - C[None, :, :].astype(np.float64)) ** 2).sum(-1)
    i = np.argsort(d, axis=1, kind="stable")[:, :m]
    return i, np.take_along_axis(d, i, 1)


def test_cpu_topk_matches_numpy_with_ties():
    """Small integers make every distance exact in float32, and centres 0/3, 1/4 and 2/5/6 are
    duplicates: the order among equal distances must be the centre index."""
    rng = np.random.default_rng(0)
    base = rng.integers(-4, 5, size=(3, 4)).astype(np.float32)
    C = np.concatenate([base, base, base[2:3]])                  # K = 7
    X = rng.integers(-4, 5, size=(40, 4)).astype(np.float32)
    for m in (1, 3, 7):
        idx, d2 = ref.topk(torch.as_tensor(X), torch.as_tensor(C), m)
        ei, ed = _np_topk(X, C, m)
        assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (40, m)
        assert np.array_equal(idx.numpy(), ei)
        assert np.array_equal(d2.numpy().astype(np.float64), ed)
    idx, d2 = ops.topk(torch.as_tensor(X), torch.as_tensor(C), 7)   # the op layer routes CPU rows here
    assert np.array_equal(idx.numpy(), _np_topk(X, C, 7)[0])
    assert (idx[:, 0] < 3).all()                                  # a duplicate never precedes its original
    for bad in (0, 8):
        with pytest.raises(ValueError):
            ops.topk(torch.as_tensor(X), torch.as_tensor(C), bad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_nonfinite_rows_and_centres_are_never_near(dtype):
    """The contract the kernels share (test_gpu_nonfinite.py): a row with a NaN or infinite
    coordinate -- one NaN, a NaN in the last column, all +inf, one -inf, one 1e20 whose square
    overflows -- gets NaN or inf distances, never 0, and changes no other row's bits; a centre
    with a NaN is the last of every row's K and in no shorter list."""
    g = torch.Generator().manual_seed(4)
    n, d, K = 70, 24, 7
    C = 8.0 * torch.randn(K, d, generator=g)
    X = (C[torch.arange(n) % K] + 0.25 * torch.randn(n, d, generator=g)).to(dtype)
    clean = X.clone()
    bad = [0, 15, 16, 35, n - 1]
    X[0, 3], X[15, d - 1], X[16], X[35, 5], X[n - 1, 7] = float("nan"), float("nan"), float("inf"), -float("inf"), 1e20
    clean[bad] = 0
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad] = False
    for squared in (True, False):
        out, exp = ops.transform(X, C, squared=squared), ops.transform(clean, C, squared=squared)
        assert not bool(torch.isfinite(out[bad]).any()) and bool(torch.isfinite(exp).all())
        assert torch.equal(out[keep].view(torch.int32), exp[keep].view(torch.int32))
    for m in (1, 3, K):
        (idx, d2), (ei, ed) = ops.topk(X, C, m), ops.topk(clean, C, m)
        assert not bool(torch.isfinite(d2[bad, 0]).any()) and int(idx.min()) >= 0 and int(idx.max()) < K
        assert torch.equal(idx[keep], ei[keep]) and torch.equal(d2[keep].view(torch.int32), ed[keep].view(torch.int32))
    for k in (0, 5, K - 1):
        C2 = C.clone()
        C2[k, 2] = float("nan")
        others = torch.arange(K) != k
        got, exp = ops.transform(clean, C2, squared=True), ops.transform(clean, C, squared=True)
        assert bool(got[:, k].isnan().all()) and torch.equal(got[:, others].view(torch.int32), exp[:, others].view(torch.int32))
        idx, d2 = ops.topk(clean, C2, K)
        ei, ed = ops.topk(clean, C, K)
        assert bool((idx[:, K - 1] == k).all()) and bool(d2[:, K - 1].isnan().all())
        for r in range(n):       # the other centres in the clean order
            assert idx[r, : K - 1].tolist() == [c for c in ei[r].tolist() if c != k]
        assert bool(torch.isfinite(d2[:, : K - 1]).all())


def test_topk_kernels_register_budget(tmp_path):
    """Every top-m instantiation keeps its lists in registers (no scratch, no spills: a list
    that moved to scratch passes every functional test, only slower), and wherever the transform
    kernel of the same (dtype, DPAD) fits two waves per SIMD (<= 256 VGPRs) so does the top-m."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    topk = _kernels("topk.hip", "topk_kernel", tmp_path)                  # (T, DPAD, P, M)
    tr = {t[:2]: r for t, r in _kernels("transform.hip", "transform_kernel", tmp_path).items()}
    assert len(tr) == 17 and {t[:2] for t in topk} == set(tr)
    for t2 in tr:   # both list sizes of every (dtype, DPAD), each with the one-block form small batches take
        assert {t[3] for t in topk if t[:2] == t2 and t[2] == "1"} == {"8", "32"}, t2
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes) for t, r in topk.items() if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
    over = [(t, r.vgprs, tr[t[:2]].vgprs) for t, r in topk.items() if tr[t[:2]].vgprs <= 256 and r.vgprs > 256]
    assert not over, over


def _fitted(n=400, d=5, k=6, **kw):
    X = torch.as_tensor(np.random.default_rng(1).normal(size=(n, d)), dtype=torch.float32)
    return X, mikmeans.KMeans(k, device="cpu", seed=1, **kw).fit(X)


def test_kmeans_predict_topk_cpu():
    X, km = _fitted()
    lab, dist = km.predict_topk(X, 3)
    assert lab.shape == dist.shape == (400, 3) and lab.dtype == torch.int32 and dist.dtype == torch.float32
    assert torch.equal(lab[:, 0], km.predict(X))
    full = km.transform(X)
    torch.testing.assert_close(dist, full.gather(1, lab.long()))
    torch.testing.assert_close(dist, full.sort(dim=1).values[:, :3])
    _, sq = km.predict_topk(X, 3, squared=True)
    torch.testing.assert_close(sq.sqrt(), dist)
    nl, nd = km.predict_topk(X.numpy(), 6)                         # numpy in, numpy out; m = K
    assert isinstance(nl, np.ndarray) and isinstance(nd, np.ndarray) and nl.shape == (400, 6)
    assert (np.sort(nl, axis=1) == np.arange(6)).all()
    for bad in (0, 7):
        with pytest.raises(ValueError):
            km.predict_topk(X, bad)
    with pytest.raises(RuntimeError):
        mikmeans.KMeans(3, device="cpu").predict_topk(X, 1)
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(X)
    ml, md = mb.predict_topk(X, 2)
    assert torch.equal(ml[:, 0], mb.predict(X)) and bool((md[:, 0] <= md[:, 1]).all())


def test_functional_predict_topk():
    X, km = _fitted()
    C = km.cluster_centers_
    lab, dist = mikmeans.predict_topk(X.numpy(), C.numpy(), 2)
    el, ed = km.predict_topk(X, 2)
    assert isinstance(lab, np.ndarray) and np.array_equal(lab, el.numpy())
    assert np.allclose(dist, ed.numpy(), rtol=1e-6, atol=1e-6)
    tl, _ = mikmeans.predict_topk(X, C, 2)
    assert torch.is_tensor(tl) and torch.equal(tl, el)
    assert "predict_topk" in mikmeans.__all__


def test_cli_predict_top(tmp_path):
    X, km = _fitted()
    km.save(tmp_path / "m")
    np.save(tmp_path / "p.npy", X.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "mikmeans", "predict", "--model", "m", "--input", "p.npy", "--top", "3",
                        "--output", "top.npy", "--distances-output", "dist.npy", "--device", "cpu"], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lab, dist = np.load(tmp_path / "top.npy"), np.load(tmp_path / "dist.npy")
    el, ed = km.predict_topk(X, 3)
    assert lab.shape == (400, 3) and lab.dtype == np.int32 and np.array_equal(lab, el.numpy())
    assert dist.shape == (400, 3) and dist.dtype == np.float32 and np.allclose(dist, ed.numpy(), rtol=1e-6)
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["counts"] == np.bincount(el[:, 0].numpy(), minlength=6).tolist()


def test_api_predict_top():
    pytest.importorskip("fastapi")
    pytest.importorskip("httpx")
    from fastapi.testclient import TestClient

    from mikmeans.models.room import Room
    from mikmeans.serve import create_app

    X, km = _fitted(k=4)
    c = TestClient(create_app(Room(seed=0), km))
    pts = X[:20].tolist()
    el, ed = km.predict_topk(X[:20], 2, squared=True)
    r = c.post("/api/predict", json={"points": pts, "top": 2})
    assert r.status_code == 200 and r.json() == {"labels": el.tolist()}
    r = c.post("/api/predict", json={"points": pts, "top": 2, "distances": True}).json()
    assert r["labels"] == el.tolist()
    assert np.allclose(np.asarray(r["distances"]), ed.numpy(), rtol=1e-6) and np.asarray(r["distances"]).shape == (20, 2)
    for bad in (0, 5, "a", 1.5, True, None):
        assert c.post("/api/predict", json={"points": pts, "top": bad}).status_code == 400, bad
    # without "top" the answer is the one-label form, as before
    labels, mind, _ = km._assign_rows(X[:20], True)
    plain = c.post("/api/predict", json={"points": pts, "distances": True}).json()
    assert plain == {"labels": labels.tolist(), "distances": mind.tolist()}
    assert c.post("/api/predict", json={"points": pts}).json() == {"labels": km.predict(X[:20]).tolist()}
