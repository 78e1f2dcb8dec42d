"""build_index / search on the CPU: the mirrors of mikmeans.ops.cpu against a NumPy brute force, the
estimators, the functional form, the CLI, world-size invariance over gloo ranks, the memory plan
and the scan kernel's resources (the GPU kernels against the existing ones: test_gpu_ivf.py)."""
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
from mikmeans.parallel import memplan, shard_range
from mikmeans.parallel.launch import spawn_local

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ints(n=600, d=6, K=7, nq=40, seed=0):
    """Small integers (every distance exact in float32), rows i and i + n/2 identical."""
    rng = np.random.default_rng(seed)
    half = rng.integers(-4, 5, size=(n // 2, d)).astype(np.float32)
    X = np.concatenate([half, half])
    C = rng.integers(-4, 5, size=(K, d)).astype(np.float32)
    Q = rng.integers(-4, 5, size=(nq, d)).astype(np.float32)
    return X, C, Q


def _np_d2(A, B):
    return ((A[:, None, :].astype(np.float64) - B[None, :, :].astype(np.float64)) ** 2).sum(-1)


def _np_search(X, C, Q, m, nprobe):
    """float64 brute force: every row's list by a stable argmin, every query's probes by a stable
    argsort, the candidates in a stable argsort (equal distances to the lower row id)."""
    lab = np.argmin(_np_d2(X, C), axis=1)
    probes = np.argsort(_np_d2(Q, C), axis=1, kind="stable")[:, :nprobe]
    D = _np_d2(Q, X)
    rows = np.full((Q.shape[0], m), -1, dtype=np.int64)
    d2 = np.full((Q.shape[0], m), np.nan)
    for q in range(Q.shape[0]):
        cand = np.flatnonzero(np.isin(lab, probes[q]))
        o = cand[np.argsort(D[q, cand], kind="stable")][:m]
        rows[q, : o.size], d2[q, : o.size] = o, D[q, o]
    return rows, d2


def test_partition_mirror_is_the_stable_argsort():
    rng = np.random.default_rng(1)
    K = 9
    lab = rng.integers(0, K, size=2000)
    lab[lab == 4] = 5                                      # an empty cluster
    lab[rng.integers(0, 2000, size=100)] = -1
    lab[rng.integers(0, 2000, size=100)] = K
    lab[rng.integers(0, 2000, size=10)] = K + 3
    valid = np.flatnonzero((lab >= 0) & (lab < K))
    exp = valid[np.argsort(lab[valid], kind="stable")]
    for t in (torch.as_tensor(lab, dtype=torch.int32), torch.as_tensor(lab)):
        order, offsets, rpos = ops.partition(t, K, want_pos=True)       # the op layer routes CPU labels here
        assert order.dtype == offsets.dtype == torch.int64 and order.shape == (2000,)
        assert np.array_equal(order[: exp.size].numpy(), exp) and bool((order[exp.size:] == -1).all())
        assert np.array_equal(offsets.numpy(), np.concatenate([[0], np.cumsum(np.bincount(lab[valid], minlength=K))]))
        assert int(offsets[5]) == int(offsets[4])
        assert np.array_equal(rpos[order[: exp.size]].numpy(), np.arange(exp.size)) and int((rpos >= 0).sum()) == exp.size
    o2, f2 = ops.partition(torch.as_tensor(lab), K)
    assert torch.equal(o2, order) and torch.equal(f2, offsets)
    with pytest.raises(ValueError):
        ops.partition(torch.as_tensor(lab), 0)


@pytest.mark.parametrize("m,nprobe", [(1, 1), (2, 3), (8, 2), (32, 7), (5, 7)])
def test_mirror_against_brute_force(m, nprobe):
    X, C, Q = _ints()
    Xt, Ct, Qt = torch.as_tensor(X), torch.as_tensor(C), torch.as_tensor(Q)
    ix = ops.index_build(Xt, Ct)
    assert not ix.native and int(ix.offsets[-1]) == X.shape[0]
    lab = np.argmin(_np_d2(X, C), axis=1)
    assert np.array_equal((ix.offsets[1:] - ix.offsets[:-1]).numpy(), np.bincount(lab, minlength=C.shape[0]))
    assert np.array_equal(ix.order.numpy(), np.argsort(lab, kind="stable"))
    keys = ops.index_search(ix, Qt, Ct, m, nprobe)
    assert keys.dtype == torch.int64 and keys.shape == (Q.shape[0], m)
    assert torch.equal(keys, ref.index_search(ix, Qt, Ct, m, nprobe))
    rows, d2 = ops.index_decode(keys)
    er, ed = _np_search(X, C, Q, m, nprobe)
    assert np.array_equal(rows.numpy(), er)
    assert np.array_equal(d2.numpy().astype(np.float64), ed, equal_nan=True)
    if m >= 2 and nprobe == C.shape[0]:
        # the nearest row's twin lies in the same list at the same distance: behind it
        assert bool((d2[:, 0] == d2[:, 1]).all()) and bool((rows[:, 0] < rows[:, 1]).all())
    # any blocking of the build, any run: the same tensors
    for other in (ops.index_build(Xt, Ct, block_rows=77), ops.index_build(Xt, Ct)):
        for name, t in ix.tensors().items():
            assert torch.equal(t, other.tensors()[name]), name


def test_rows_without_a_finite_distance_are_in_no_list():
    X, C, Q = _ints()
    X[7] = np.inf
    X[11, 2] = np.nan
    ix = ops.index_build(torch.as_tensor(X), torch.as_tensor(C))
    assert int(ix.offsets[-1]) == X.shape[0] - 2
    assert not ({7, 11} & set(ix.order.tolist())) and ix.order[-2:].tolist() == [-1, -1]
    rows, _ = ops.index_decode(ops.index_search(ix, torch.as_tensor(Q), torch.as_tensor(C), 32, C.shape[0]))
    assert not ({7, 11} & set(rows.flatten().tolist()))


def _fitted(n=600, d=6, K=7, **kw):
    X, _, Q = _ints(n, d, K)
    X, Q = torch.as_tensor(X), torch.as_tensor(Q)
    return X, Q, mikmeans.KMeans(K, device="cpu", seed=1, **kw).fit(X)


def test_estimator_build_index_and_search_cpu():
    X, Q, km = _fitted()
    K = km.n_clusters
    ix = km.build_index(X)
    assert isinstance(ix, mikmeans.ClusterIndex) and ix.n_rows == 600
    lab = km.predict_topk(X, 1)[0][:, 0].long()
    assert ix.list_sizes.dtype == ix.offsets.dtype == ix.order.dtype == torch.int64
    assert torch.equal(ix.list_sizes, torch.bincount(lab, minlength=K)) and ix.offsets.shape == (K + 1,)
    assert torch.equal(ix.order, torch.sort(lab, stable=True).indices)
    for k in range(K):
        assert torch.equal(ix.rows_of(k), (lab == k).nonzero().flatten())
    with pytest.raises(ValueError):
        ix.rows_of(K)
    assert ix.nbytes == sum(t.numel() * t.element_size() for t in ix._index.tensors().values()) > 0
    # nprobe = K is the brute force over the indexed rows
    rows, dist = ix.search(Q, 5, nprobe=K)
    assert rows.shape == dist.shape == (40, 5) and rows.dtype == torch.int64 and dist.dtype == torch.float32
    er, ed = _np_search(X.numpy(), km.cluster_centers_.numpy(), Q.numpy(), 5, K)
    assert np.array_equal(rows.numpy(), er)
    _, sq = ix.search(Q, 5, nprobe=K, squared=True)
    assert np.array_equal(sq.numpy().astype(np.float64), ed) and torch.equal(dist, sq.sqrt())
    # fewer probes: a subset of the rows, never nearer than the exact answer
    r1, d1 = ix.search(Q, 5, nprobe=1)
    assert bool((d1 >= dist).all()) and torch.equal(lab[r1[:, 0]], km.predict_topk(Q, 1)[0][:, 0].long())
    # numpy in, numpy out
    nr, nd = ix.search(Q.numpy(), 5, nprobe=K)
    assert isinstance(nr, np.ndarray) and isinstance(nd, np.ndarray) and nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nr, rows.numpy()) and np.array_equal(nd, dist.numpy())
    hx = km.build_index(X.numpy())
    assert torch.equal(hx.order, ix.order)
    two = ix.search(Q, 5, nprobe=3)
    again = ix.search(Q, 5, nprobe=3)
    assert torch.equal(two[0], again[0]) and torch.equal(two[1], again[1])


def test_search_pads_with_minus_one_and_nan():
    X, Q, km = _fitted()
    km.cluster_centers_[2] = 1e6                          # an empty cluster ...
    ix = km.build_index(X)
    assert int(ix.list_sizes[2]) == 0 and ix.rows_of(2).numel() == 0
    far = torch.full((1, X.shape[1]), 1e6)                # ... and a query that probes only it
    rows, dist = ix.search(torch.cat([far, Q]), 4, nprobe=1)
    assert rows[0].tolist() == [-1] * 4 and bool(dist[0].isnan().all())
    assert bool((rows[1:] >= 0).all()) and not bool(dist[1:].isnan().any())
    none = km.build_index(X[:0])                          # no rows at all
    rows, dist = none.search(Q, 2, nprobe=3)
    assert none.n_rows == 0 and none.order.numel() == 0 and bool((rows == -1).all()) and bool(dist.isnan().all())
    small = km.build_index(X[:3])                         # fewer rows than m
    rows, dist = small.search(Q, 8, nprobe=km.n_clusters)
    assert bool((rows[:, :3] >= 0).all()) and bool((rows[:, 3:] == -1).all()) and bool(dist[:, 3:].isnan().all())


def test_limits_and_unfitted_raise():
    X, Q, km = _fitted()
    ix = km.build_index(X)
    for m, nprobe in ((0, 1), (33, 1), (4, 0), (4, km.n_clusters + 1)):
        with pytest.raises(ValueError):
            ix.search(Q, m, nprobe=nprobe)
        with pytest.raises(ValueError):
            ops.index_search(ix._index, Q, km.cluster_centers_, m, nprobe)
    with pytest.raises(ValueError):
        ix.search(Q[:, :3], 4)                            # another width
    with pytest.raises(RuntimeError):
        mikmeans.KMeans(3, device="cpu").build_index(X)


def test_cosine_model_indexes_unit_rows():
    rng = np.random.default_rng(5)
    X = torch.as_tensor(rng.normal(size=(500, 8)), dtype=torch.float32)
    Q = torch.as_tensor(rng.normal(size=(30, 8)), dtype=torch.float32)
    km = mikmeans.KMeans(6, metric="cosine", device="cpu", seed=0).fit(X)
    K = km.n_clusters
    rows, dist = km.build_index(X).search(Q, 3, nprobe=K)
    rows5, dist5 = km.build_index(5.0 * X).search(0.5 * Q, 3, nprobe=K)          # scale-free
    assert torch.equal(rows, rows5)
    torch.testing.assert_close(dist, dist5)
    Xu, Qu = X / X.norm(dim=1, keepdim=True), Q / Q.norm(dim=1, keepdim=True)
    exp = torch.cdist(Qu.double(), Xu.double())
    best = exp.sort(dim=1).values[:, :3]
    torch.testing.assert_close(dist.double(), best, atol=1e-3, rtol=1e-3)


def test_minibatch_and_functional_forms():
    X, Q, km = _fitted()
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(X)
    rows, sq = mb.build_index(X).search(Q, 3, nprobe=4, squared=True)
    er, ed = _np_search(X.numpy(), mb.cluster_centers_.numpy(), Q.numpy(), 3, 4)
    assert np.array_equal(rows.numpy(), er) and np.array_equal(sq.numpy().astype(np.float64), ed)
    assert "build_index" in mikmeans.__all__ and "ClusterIndex" in mikmeans.__all__
    C = km.cluster_centers_
    fx = mikmeans.build_index(X.numpy(), C.numpy())
    assert isinstance(fx, mikmeans.ClusterIndex)
    fr, fd = fx.search(Q.numpy(), 4, nprobe=2)
    kr, kd = km.build_index(X).search(Q, 4, nprobe=2)
    assert isinstance(fr, np.ndarray) and np.array_equal(fr, kr.numpy()) and np.array_equal(fd, kd.numpy())


def test_cli_search(tmp_path):
    X, Q, km = _fitted()
    km.save(tmp_path / "m")
    np.save(tmp_path / "x.npy", X.numpy())
    np.save(tmp_path / "q.npy", Q.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "mikmeans", "search", "--model", "m", "--input", "x.npy", "--queries", "q.npy",
            "--device", "cpu"]
    r = subprocess.run([*base, "--top", "4", "--nprobe", "3", "--output", "out.npz"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows, dist = km.build_index(X).search(Q, 4, nprobe=3)
    got = np.load(tmp_path / "out.npz")
    assert got["rows"].dtype == np.int64 and got["distances"].dtype == np.float32
    assert np.array_equal(got["rows"], rows.numpy()) and np.array_equal(got["distances"], dist.numpy())
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"n_samples": 600, "n_queries": 40, "top": 4, "nprobe": 3,
                                                             "found": 160}
    r = subprocess.run([*base, "--top", "2", "--squared", "--output", "sq.npz"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)                # (--nprobe defaults to 8 > K = 7)
    assert r.returncode != 0 and "--nprobe" in r.stderr
    r = subprocess.run([*base, "--top", "2", "--nprobe", "7", "--squared", "--output", "sq.npz"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, sq = km.build_index(X).search(Q, 2, nprobe=7, squared=True)
    assert np.array_equal(np.load(tmp_path / "sq.npz")["distances"], sq.numpy())


WS_N, WS_K, WS_M = 1201, 6, 5


def _ws_search(comm):
    X, C, Q = _ints(WS_N - 1, 6, WS_K, nq=50, seed=12)
    X = torch.as_tensor(np.concatenate([X, X[:1]]))
    X[5] = float("inf")                                               # (a row no list holds)
    C = torch.as_tensor(C)
    C[3] = 1e6                                                        # (an empty cluster)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    ix = km.build_index(X[s:e])
    out = {"order": ix.order, "first": s}
    for nprobe in (1, 2, WS_K):
        out[nprobe] = ix.search(torch.as_tensor(Q), WS_M, nprobe=nprobe)
    return out


def test_search_is_world_size_invariant():
    from mikmeans.parallel import Comm

    one = _ws_search(Comm.local())
    rows, dist = one[WS_K]
    assert 5 not in rows.flatten().tolist() and int(rows.max()) > WS_N * 2 // 3     # rows of the last shard are found
    assert bool((rows[:, 1:][dist[:, 1:] == dist[:, :-1]] > rows[:, :-1][dist[:, 1:] == dist[:, :-1]]).all())
    for world in (2, 3):
        outs = spawn_local(_ws_search, world)
        for o in outs:
            for nprobe in (1, 2, WS_K):
                assert torch.equal(o[nprobe][0], one[nprobe][0])
                assert torch.equal(o[nprobe][1].view(torch.int32), one[nprobe][1].view(torch.int32))   # (bits: NaN == NaN)
            assert bool((o["order"] >= o["first"]).all())                               # global row ids
        assert sorted(torch.cat([o["order"] for o in outs]).tolist()) == sorted(one["order"].tolist())


@pytest.mark.parametrize("n,D,K,dtype", [(600, 6, 7, torch.float32), (1000, 30, 37, torch.bfloat16),
                                         (50, 1100, 3, torch.float32)])
def test_plan_index_lists_the_index_tensors(n, D, K, dtype):
    g = torch.Generator().manual_seed(0)
    X = torch.randn(n, D, generator=g).to(dtype)
    C = torch.randn(K, D, generator=g)
    ix = ops.index_build(X, C)
    plan = memplan.plan_index(n, D, K, dtype)
    es = 2 if dtype == torch.bfloat16 else 4
    assert plan.mode == "index" and set(plan.persistent) == set(ix.tensors())
    for name, t in ix.tensors().items():
        if name == "row_pack":          # (CPU rows keep their own width; the plan counts the kernels' padded one)
            cols = memplan.dpad_for(memplan.padded_cols(D, es), es) or memplan.padded_cols(D, es)
            assert plan.persistent[name] == memplan._r(ops.index_tiles(n, K) * 16 * cols * es)
            assert t.numel() == ops.index_tiles(n, K) * 16 * ix.cols and ix.cols <= cols
        else:
            assert plan.persistent[name] == memplan._r(t.numel() * t.element_size()), name
    assert {"labels", "row_pos", "top1_idx", "top1_d2", "partition_cells"} <= set(plan.transient["build"])
    assert plan.peak == plan.persistent_bytes + sum(plan.transient["build"].values())
    plan.budget = plan.peak - 1
    assert not plan.fits


def test_plan_mirrors_the_native_partition_geometry():
    from mikmeans.ops import native

    if not native.available():
        pytest.skip("native extension not built")
    C = native.require()
    assert C.PARTITION_MAX_K == ops.PARTITION_MAX_K == ref.PARTITION_MAX_K
    assert C.IVF_EMPTY_KEY == ops.IVF_EMPTY_KEY
    for n, K in ((0, 1), (1, 1), (1023, 7), (1025, 7), (10**7, 1024), (10**7, 10240), (5000, 4097), (2**31, 3)):
        assert memplan.partition_blocks(n, K) == C.partition_blocks(n, K), (n, K)


def test_scan_kernels_register_budget(tmp_path):
    """Every scan instantiation keeps its lists in registers (no scratch, no spills) and fits two
    waves per SIMD (<= 256 VGPRs) wherever topk_kernel of the same (T, DPAD, P, M) does; the scan
    has exactly topk's instantiations."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    assert "ivf.hip" in _build.HIP_SOURCES
    scan = _kernels("ivf.hip", "ivf_scan_kernel", tmp_path)               # (T, DPAD, P, M)
    topk = _kernels("topk.hip", "topk_kernel", tmp_path)
    assert set(scan) == set(topk) and len(scan) > 34
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes) for t, r in scan.items() if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
    over = [(t, r.vgprs, topk[t].vgprs) for t, r in scan.items() if topk[t].vgprs <= 256 and r.vgprs > 256]
    assert not over, over
