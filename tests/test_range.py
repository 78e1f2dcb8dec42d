"""range_search / range_count on the CPU: the mirror of mikmeans.ops.cpu against a float64 brute
force on integer data, the estimators, the functional form, the CLI, world-size invariance over
gloo ranks and the range kernels' resources (the GPU kernels against the existing ones:
test_gpu_range.py)."""
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
from mikmeans.parallel import shard_range
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


def _np_range(X, C, Q, r2, nprobe, sort=True):
    """float64 brute force: every row's list by a stable argmin, every query's probes by a stable
    argsort, the hits d2 <= r2[q] in a stable argsort (equal distances to the lower row id), or probe
    after probe and ascending row within a probe."""
    lab = np.argmin(_np_d2(X, C), axis=1)
    probes = np.argsort(_np_d2(Q, C), axis=1, kind="stable")[:, :nprobe]
    D = _np_d2(Q, X)
    lims, rows, d2 = [0], [], []
    for q in range(Q.shape[0]):
        if sort:
            cand = np.flatnonzero(np.isin(lab, probes[q]) & (D[q] <= r2[q]))
            cand = cand[np.argsort(D[q, cand], kind="stable")]
        else:
            cand = np.concatenate([np.flatnonzero((lab == k) & (D[q] <= r2[q])) for k in probes[q]])
        rows.append(cand)
        d2.append(D[q, cand])
        lims.append(lims[-1] + cand.size)
    return np.array(lims, dtype=np.int64), np.concatenate(rows).astype(np.int64), np.concatenate(d2)


def _radii(nq):
    return np.array([0.0, 9.0, 25.0, 60.0, 1e6], dtype=np.float32)[np.arange(nq) % 5]


@pytest.mark.parametrize("nprobe", [1, 3, 7])
@pytest.mark.parametrize("sort", [True, False])
def test_mirror_against_brute_force(nprobe, sort):
    X, C, Q = _ints()
    Xt, Ct, Qt = torch.as_tensor(X), torch.as_tensor(C), torch.as_tensor(Q)
    ix = ops.index_build(Xt, Ct)
    r2 = _radii(Q.shape[0])
    lims, keys = ops.index_range(ix, Qt, Ct, torch.as_tensor(r2), nprobe, sort=sort)
    assert lims.dtype == keys.dtype == torch.int64 and lims.shape == (Q.shape[0] + 1,)
    again = ref.index_range(ix, Qt, Ct, torch.as_tensor(r2), nprobe, sort=sort)
    assert torch.equal(lims, again[0]) and torch.equal(keys, again[1])
    rows, d2 = ops.index_decode(keys)
    el, er, ed = _np_range(X, C, Q, r2, nprobe, sort)
    assert np.array_equal(lims.numpy(), el) and np.array_equal(rows.numpy(), er)
    assert np.array_equal(d2.numpy().astype(np.float64), ed)
    counts = ops.index_range(ix, Qt, Ct, torch.as_tensor(r2), nprobe, count_only=True)
    assert counts.dtype == torch.int64 and torch.equal(counts, lims[1:] - lims[:-1])
    cnt = np.diff(el)
    assert (cnt[0::5] <= cnt[4::5]).all() and cnt[4::5].sum() > 0 and 0 < cnt.sum() < cnt.size * X.shape[0]
    # the probe ranks of the hits: the probed list's place among the query's probes
    _, k2, pr = ops.index_range(ix, Qt, Ct, torch.as_tensor(r2), nprobe, sort=sort, want_probe=True)
    lab = np.argmin(_np_d2(X, C), axis=1)
    probes = np.argsort(_np_d2(Q, C), axis=1, kind="stable")[:, :nprobe]
    qid = np.repeat(np.arange(Q.shape[0]), cnt)
    assert torch.equal(k2, keys) and np.array_equal(probes[qid, pr.numpy()], lab[er])
    # a scalar radius is every query's
    l1, k1 = ops.index_range(ix, Qt, Ct, 25.0, nprobe, sort=sort)
    e1 = _np_range(X, C, Q, np.full(Q.shape[0], 25.0), nprobe, sort)
    assert np.array_equal(l1.numpy(), e1[0]) and np.array_equal(ops.index_decode(k1)[0].numpy(), e1[1])


def test_rows_in_no_list_and_nonfinite_queries_have_no_hits():
    X, C, Q = _ints()
    X[7] = np.inf
    X[11, 2] = np.nan
    Q2 = Q.copy()
    Q2[3, 1] = np.nan
    Q2[8, 0] = np.inf
    Xt, Ct = torch.as_tensor(X), torch.as_tensor(C)
    ix = ops.index_build(Xt, Ct)
    K = C.shape[0]
    lims, keys = ops.index_range(ix, torch.as_tensor(Q), Ct, 1e6, K)
    rows, _ = ops.index_decode(keys)
    assert not ({7, 11} & set(rows.tolist())) and bool((lims[1:] - lims[:-1] == X.shape[0] - 2).all())
    l2, k2 = ops.index_range(ix, torch.as_tensor(Q2), Ct, 40.0, K)
    l1, k1 = ops.index_range(ix, torch.as_tensor(Q), Ct, 40.0, K)
    assert int(l2[4] - l2[3]) == 0 and int(l2[9] - l2[8]) == 0
    for q in range(Q.shape[0]):
        if q not in (3, 8):
            assert torch.equal(k2[l2[q] : l2[q + 1]], k1[l1[q] : l1[q + 1]]), q


def _fitted(n=600, d=6, K=7, **kw):
    X, _, Q = _ints(n, d, K)
    X, Q = torch.as_tensor(X), torch.as_tensor(Q)
    return X, Q, mikmeans.KMeans(K, device="cpu", seed=1, **kw).fit(X)


def test_estimator_range_search_cpu():
    X, Q, km = _fitted()
    K = km.n_clusters
    ix = km.build_index(X)
    assert hasattr(mikmeans.ClusterIndex, "range_search") and hasattr(mikmeans.ClusterIndex, "range_count")
    C = km.cluster_centers_.numpy()
    r = np.sqrt(_radii(Q.shape[0])).astype(np.float32)
    r2 = r * r                                                  # (float32 products, as the method squares)
    lims, rows, dist = ix.range_search(Q, r, nprobe=K)
    assert lims.dtype == rows.dtype == torch.int64 and dist.dtype == torch.float32
    el, er, ed = _np_range(X.numpy(), C, Q.numpy(), r2, K)
    assert np.array_equal(lims.numpy(), el) and np.array_equal(rows.numpy(), er)
    _, _, sq = ix.range_search(Q, r2, nprobe=K, squared=True)
    assert np.array_equal(sq.numpy().astype(np.float64), ed) and torch.equal(dist, sq.sqrt())
    # unsorted: the same hits per query, probe after probe and ascending within a probe
    ul, ur, ud = ix.range_search(Q, r, nprobe=3, sort=False)
    el, er, ed = _np_range(X.numpy(), C, Q.numpy(), r2, 3, sort=False)
    assert np.array_equal(ul.numpy(), el) and np.array_equal(ur.numpy(), er)
    assert np.array_equal((ud * ud).round().numpy().astype(np.float64), ed)
    counts = ix.range_count(Q, r, nprobe=3)
    assert counts.dtype == torch.int64 and torch.equal(counts, ul[1:] - ul[:-1])
    # a scalar radius; numpy in, numpy out; the same from run to run
    sl, sr, sd = ix.range_search(Q, 4.0, nprobe=2)
    nl, nr, nd = ix.range_search(Q.numpy(), 4.0, nprobe=2)
    assert all(isinstance(t, np.ndarray) for t in (nl, nr, nd)) and nl.dtype == nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nl, sl.numpy()) and np.array_equal(nr, sr.numpy()) and np.array_equal(nd, sd.numpy())
    nc = ix.range_count(Q.numpy(), 4.0, nprobe=2)
    assert isinstance(nc, np.ndarray) and nc.dtype == np.int64 and np.array_equal(nc, np.diff(nl))
    # the follow-up to a search: everything at least as close as the m-th neighbour
    m = 5
    kr, kd = ix.search(Q, m, nprobe=K, squared=True)
    fl, fr, fd = ix.range_search(Q, kd[:, m - 1], nprobe=K, squared=True)
    for q in range(Q.shape[0]):
        a, b = int(fl[q]), int(fl[q + 1])
        assert b - a >= m and torch.equal(fr[a : a + m], kr[q]) and torch.equal(fd[a : a + m], kd[q])
        assert bool((fd[a + m : b] == kd[q, m - 1]).all())
    # max_results: the total passes, one less raises and names the total
    total = int(sl[-1])
    assert total > 0 and int(ix.range_search(Q, 4.0, nprobe=2, max_results=total)[0][-1]) == total
    with pytest.raises(ValueError, match=str(total)):
        ix.range_search(Q, 4.0, nprobe=2, max_results=total - 1)
    none = km.build_index(X[:0])                                  # no rows at all
    zl, zr, zd = none.range_search(Q, 1e3, nprobe=3)
    assert bool((zl == 0).all()) and zl.shape == (Q.shape[0] + 1,) and zr.numel() == 0 and zd.numel() == 0
    assert bool((none.range_count(Q, 1e3, nprobe=3) == 0).all())


def test_bad_arguments_raise():
    X, Q, km = _fitted()
    ix = km.build_index(X)
    K = km.n_clusters
    nq = Q.shape[0]
    for radius in (-1.0, float("nan"), float("inf"), np.ones(nq - 1), np.ones((nq, 1)), [1.0, -1.0] * (nq // 2), 1e30):
        with pytest.raises(ValueError):
            ix.range_search(Q, radius, nprobe=2)
        with pytest.raises(ValueError):
            ix.range_count(Q, radius, nprobe=2)
    assert int(ix.range_search(Q, 1e30, nprobe=2, squared=True)[0][-1]) > 0     # (finite as a squared radius)
    for nprobe in (0, K + 1):
        with pytest.raises(ValueError):
            ix.range_search(Q, 1.0, nprobe=nprobe)
        with pytest.raises(ValueError):
            ix.range_count(Q, 1.0, nprobe=nprobe)
        with pytest.raises(ValueError):
            ops.index_range(ix._index, Q, km.cluster_centers_, 1.0, nprobe)
    with pytest.raises(ValueError):
        ix.range_search(Q[0], 1.0, nprobe=2)                      # not 2-D
    with pytest.raises(ValueError):
        ix.range_search(Q[:, :3], 1.0, nprobe=2)                  # another width
    with pytest.raises(ValueError):
        ops.index_range(ix._index, Q, km.cluster_centers_, -1.0, 2)


def test_minibatch_functional_and_cosine_forms():
    X, Q, km = _fitted()
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(X)
    lims, rows, sq = mb.build_index(X).range_search(Q, 30.0, nprobe=4, squared=True)
    el, er, ed = _np_range(X.numpy(), mb.cluster_centers_.numpy(), Q.numpy(), np.full(Q.shape[0], 30.0), 4)
    assert np.array_equal(lims.numpy(), el) and np.array_equal(rows.numpy(), er)
    assert np.array_equal(sq.numpy().astype(np.float64), ed)
    assert "index_range" in ops.__all__ and ops.index_range is not None
    C = km.cluster_centers_
    fx = mikmeans.build_index(X.numpy(), C.numpy())
    fl, fr, fd = fx.range_search(Q.numpy(), 4.0, nprobe=2)
    kl, kr, kd = km.build_index(X).range_search(Q, 4.0, nprobe=2)
    assert isinstance(fr, np.ndarray) and np.array_equal(fl, kl.numpy()) and np.array_equal(fr, kr.numpy())
    assert np.array_equal(fd, kd.numpy())
    rng = np.random.default_rng(5)
    Xc = torch.as_tensor(rng.normal(size=(500, 8)), dtype=torch.float32)
    Qc = torch.as_tensor(rng.normal(size=(30, 8)), dtype=torch.float32)
    cm = mikmeans.KMeans(6, metric="cosine", device="cpu", seed=0).fit(Xc)
    cl, cr, cd = cm.build_index(Xc).range_search(Qc, 0.9, nprobe=6)
    l5, r5, _ = cm.build_index(5.0 * Xc).range_search(0.5 * Qc, 0.9, nprobe=6)      # scale-free: unit rows
    exp = torch.cdist(Qc / Qc.norm(dim=1, keepdim=True), Xc / Xc.norm(dim=1, keepdim=True))
    near = ((exp - 0.9).abs() < 1e-4).any(dim=1)                  # (queries with a row on the boundary)
    assert int(cl[-1]) > 0 and bool((cd <= 0.9 + 1e-6).all())
    assert torch.equal((cl[1:] - cl[:-1])[~near], (exp <= 0.9).sum(1)[~near])
    assert torch.equal((l5[1:] - l5[:-1])[~near], (cl[1:] - cl[:-1])[~near])


def test_native_source_is_listed():
    from mikmeans import _build

    assert "range.hip" in _build.HIP_SOURCES and (_build.CSRC / "range.hip").exists()


def test_cli_search_radius(tmp_path):
    X, Q, km = _fitted()
    km.save(tmp_path / "m")
    np.save(tmp_path / "x.npy", X.numpy())
    np.save(tmp_path / "q.npy", Q.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "mikmeans", "search", "--model", "m", "--input", "x.npy", "--queries", "q.npy",
            "--device", "cpu"]
    r = subprocess.run([*base, "--radius", "4", "--nprobe", "3", "--output", "out.npz"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lims, rows, dist = km.build_index(X).range_search(Q, 4.0, nprobe=3)
    got = np.load(tmp_path / "out.npz")
    assert sorted(got.files) == ["distances", "lims", "rows"]
    assert got["lims"].dtype == got["rows"].dtype == np.int64 and got["distances"].dtype == np.float32
    assert np.array_equal(got["lims"], lims.numpy()) and np.array_equal(got["rows"], rows.numpy())
    assert np.array_equal(got["distances"], dist.numpy())
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"n_samples": 600, "n_queries": 40, "radius": 4.0,
                                                             "nprobe": 3, "found": int(lims[-1])}
    r = subprocess.run([*base, "--radius", "16", "--nprobe", "7", "--squared", "--output", "sq.npz"], cwd=tmp_path,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    _, sr, sq = km.build_index(X).range_search(Q, 16.0, nprobe=7, squared=True)
    got = np.load(tmp_path / "sq.npz")
    assert np.array_equal(got["rows"], sr.numpy()) and np.array_equal(got["distances"], sq.numpy())
    for extra in (["--radius", "4", "--top", "2"], [], ["--radius", "-1"]):     # both, neither, a negative radius
        r = subprocess.run([*base, *extra, "--nprobe", "3"], cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode != 0 and ("--radius" in r.stderr)


WS_N, WS_K = 1201, 6


def _ws_range(comm):
    X, C, Q = _ints(WS_N - 1, 6, WS_K, nq=50, seed=12)
    X = torch.as_tensor(np.concatenate([X, X[:1]]))
    X[5] = float("inf")                                               # (a row no list holds)
    C = torch.as_tensor(C)
    C[3] = 1e6                                                        # (an empty cluster)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    ix = km.build_index(X[s:e])
    Q = torch.as_tensor(Q)
    r2 = torch.as_tensor(_radii(Q.shape[0]))
    out = {}
    for nprobe in (1, 2, WS_K):
        for sort in (True, False):
            out[f"{nprobe}{sort}"] = ix.range_search(Q, r2, nprobe=nprobe, squared=True, sort=sort)
        out[f"{nprobe}count"] = ix.range_count(Q, r2, nprobe=nprobe, squared=True)
    try:
        ix.range_search(Q, r2, nprobe=WS_K, squared=True, max_results=3)
        out["raised"] = ""
    except ValueError as err:
        out["raised"] = str(err)
    return out


def test_range_search_is_world_size_invariant():
    from mikmeans.parallel import Comm

    one = _ws_range(Comm.local())
    lims, rows, d2 = one[f"{WS_K}True"]
    assert 5 not in rows.tolist() and int(rows.max()) > WS_N * 2 // 3           # rows of the last shard are found
    assert int(lims[-1]) > 3 * 50 and str(int(lims[-1])) in one["raised"]
    same = d2[1:] == d2[:-1]                                                    # (exact ties: the twins)
    inner = torch.ones(rows.numel(), dtype=torch.bool)
    inner[lims[1:-1][lims[1:-1] < rows.numel()]] = False                       # (not across two queries)
    assert int((same & inner[1:]).sum()) > 0 and bool((rows[1:] > rows[:-1])[same & inner[1:]].all())
    ul, ur, _ = one[f"{WS_K}False"]
    assert torch.equal(ul, lims) and sorted(ur.tolist()) == sorted(rows.tolist()) and not torch.equal(ur, rows)
    for world in (2, 3):
        for o in spawn_local(_ws_range, world):
            for nprobe in (1, 2, WS_K):
                for sort in (True, False):
                    for got, exp in zip(o[f"{nprobe}{sort}"], one[f"{nprobe}{sort}"]):
                        assert got.dtype == exp.dtype and torch.equal(got, exp), (world, nprobe, sort)
                assert torch.equal(o[f"{nprobe}count"], one[f"{nprobe}count"])
                assert torch.equal(o[f"{nprobe}count"], one[f"{nprobe}True"][0][1:] - one[f"{nprobe}True"][0][:-1])
            assert o["raised"] == one["raised"]


def test_range_kernels_register_budget(tmp_path):
    """Every instantiation of the count and the fill kernel runs without scratch or spills in at
    most 256 VGPRs (two waves per SIMD), and both cover every (dtype, padded width) of the scan."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    rng = _kernels("range.hip", "ivf_range_kernel", tmp_path)             # (T, DPAD, P, FILL)
    scan = _kernels("ivf.hip", "ivf_scan_kernel", tmp_path)               # (T, DPAD, P, M)
    widths = {t[:2] for t in scan}
    assert len(widths) >= 17
    for fill in ("true", "false"):
        assert {t[:2] for t in rng if t[3] == fill} == widths, fill
        assert {t[:2] for t in rng if t[3] == fill and t[2] == "1"} == widths, fill    # the small-batch form
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes) for t, r in rng.items()
           if r.vgpr_spills or r.scratch_bytes or r.vgprs > 256]
    assert not bad, bad
