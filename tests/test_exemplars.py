"""cluster_exemplars on the CPU: the integer mirror of csrc/exemplars.hip against a NumPy lexsort
per cluster, split freedom, the estimators, the functional form, the CLI's ``report --exemplars``,
world-size invariance over gloo ranks and the kernel's resources (the GPU kernel against this
mirror: test_gpu_exemplars.py)."""
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
from mikmeans.api import _jsonable
from mikmeans.ops import cpu as ref
from mikmeans.parallel import shard_range
from mikmeans.parallel.launch import spawn_local

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def brute_force(idx, d2, K, m, row0=0, farthest=False):
    """(rows int64 [K, m], d2 float32 [K, m]) by a NumPy lexsort of every cluster's rows."""
    k = idx[:, 0].cpu().numpy().astype(np.int64)
    d = d2[:, 0].cpu().numpy().astype(np.float32)
    rows = np.full((K, m), -1, dtype=np.int64)
    dist = np.full((K, m), np.nan, dtype=np.float32)
    for c in range(K):
        sel = np.nonzero((k == c) & np.isfinite(d))[0]
        a2 = np.maximum(d[sel], np.float32(0)) + np.float32(0)            # (-0 -> +0)
        o = np.lexsort((sel, -a2 if farthest else a2))[:m]
        rows[c, : len(o)] = sel[o] + row0
        dist[c, : len(o)] = a2[o]
    return rows, dist


def assert_lists(rows, d2, exp_rows, exp_d2):
    """Rows equal, distances equal as bit patterns (padded slots hold NaN)."""
    rows, d2 = np.asarray(rows.cpu() if torch.is_tensor(rows) else rows), np.asarray(d2.cpu() if torch.is_tensor(d2) else d2)
    assert rows.dtype == np.int64 and d2.dtype == np.float32 and rows.shape == d2.shape == exp_rows.shape
    assert np.array_equal(rows, exp_rows), np.argwhere(rows != exp_rows)[:8]
    assert np.array_equal(d2.view(np.int32), exp_d2.view(np.int32)), np.argwhere(d2.view(np.int32) != exp_d2.view(np.int32))[:8]


def hard_input(n=3000, K=6, seed=0):
    """(idx, d2): distances from {0, 1, 2, 4} only (ties by row), -0.0 beside 0.0, NaN / +-inf
    rows, labels -1 and K, cluster 4 without a row and cluster 5 with three."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(0, 4, (n,), generator=g).to(torch.int32)
    d = torch.tensor([0.0, 1.0, 2.0, 4.0])[torch.randint(0, 4, (n,), generator=g)]
    d[3::11] = -0.0
    d[5::37] = NAN
    d[6::41] = INF
    d[7::43] = -INF
    k[8::29] = -1
    k[9::31] = K
    k[[100, 200, 300]] = 5
    d[100], d[200], d[300] = 2.0, -0.0, 2.0
    return torch.stack([k, (k + 1) % K], 1).contiguous(), torch.stack([d, d + 1], 1).contiguous()


@pytest.mark.parametrize("farthest", [False, True])
@pytest.mark.parametrize("m", [1, 5, 64])
def test_mirror_against_brute_force(m, farthest):
    K = 6
    idx, d2 = hard_input()
    T = ref.exemplar_table(idx, d2, K, m, farthest=farthest)
    assert T.shape == (K, m) and T.dtype == torch.int64
    rows, dd = ops.exemplar_decode(T, farthest=farthest)
    exp_rows, exp_d2 = brute_force(idx, d2, K, m, farthest=farthest)
    assert_lists(rows, dd, exp_rows, exp_d2)
    assert bool((T[4] == -1).all()) and int((rows[5] >= 0).sum()) == min(m, 3)
    assert not np.signbit(dd.numpy()[np.isfinite(dd.numpy())]).any()        # -0 counted as +0
    if m == 64:
        # the -0.0 row of cluster 5 ties with nothing; the two 2.0 rows tie by row
        assert rows[5, :3].tolist() == ([100, 300, 200] if farthest else [200, 100, 300])
    # the slots are the ascending keys; row0 shifts the rows only
    keys = T[T != -1]
    assert bool((keys >= 0).all()) and all(bool((T[c, :-1][T[c, 1:] != -1] < T[c, 1:][T[c, 1:] != -1]).all()) for c in range(K))
    big = 4_000_000_000                                                   # (row indices past 2^31)
    r7, d7 = ops.exemplar_decode(ref.exemplar_table(idx, d2, K, m, row0=big, farthest=farthest), farthest=farthest,
                                 row_start=5)
    assert_lists(r7, d7, *brute_force(idx, d2, K, m, row0=big + 5, farthest=farthest))


@pytest.mark.parametrize("farthest", [False, True])
def test_table_is_split_and_order_free(farthest):
    K, m = 6, 9
    idx, d2 = hard_input(n=4000, seed=1)
    T = ref.exemplar_table(idx, d2, K, m, farthest=farthest)
    starts = list(range(0, idx.shape[0], 777))
    for order in (starts, starts[::-1]):
        acc = ops.exemplar_new(K, m)
        for s in order:
            ops.exemplar_accumulate(acc, idx[s : s + 777], d2[s : s + 777], row0=s, farthest=farthest)
        assert torch.equal(acc, T)
    # accumulating the same rows again changes nothing; merging with an empty table neither
    ops.exemplar_accumulate(acc, idx[:777], d2[:777], row0=0, farthest=farthest)
    assert torch.equal(acc, T) and torch.equal(ref.exemplar_merge(T, ops.exemplar_new(K, m)), T)
    with pytest.raises(ValueError):
        ops.exemplar_accumulate(torch.zeros((K, 65), dtype=torch.int64), idx, d2)
    with pytest.raises(ValueError):
        ops.exemplar_accumulate(acc, idx, d2, row0=(1 << 32) - 10)
    with pytest.raises(ValueError):
        ref.exemplar_table(idx, d2[:, :1], K, m)


EMPTY64 = (1 << 64) - 1


def _insert_steps(L, m, key):
    """csrc/exemplars.hip exemplar_insert as a coroutine: one access to the shared list per
    step (the read of the last slot, then the atomic min), so a scheduler can interleave
    threads between any two and every read may be stale by the time it is used."""
    for j in range(m):
        last = L[m - 1]
        yield
        if key >= last:
            return
        old = L[j]
        L[j] = min(old, key)
        yield
        if old == key:
            return
        key = max(old, key)
        if key == EMPTY64:
            return


@pytest.mark.parametrize("m", [1, 3, 8])
def test_insertion_chain_under_random_interleavings(m):
    """Whatever the interleaving, the list ends as the m smallest keys in order."""
    import random

    rng = random.Random(m)
    for trial in range(60):
        n = rng.choice([1, m, m + 1, 40])
        keys = rng.sample(range(1000), n)
        L = [EMPTY64] * m
        if trial % 3 == 0:                                                # a list that already holds keys
            L = sorted(rng.sample(range(1000, 2000), m))
            keys_all = keys + L
        else:
            keys_all = keys
        live = [_insert_steps(L, m, k) for k in keys]
        while live:
            t = rng.randrange(len(live)) if trial % 2 else 0              # (odd trials: random; even: one by one)
            try:
                next(live[t])
            except StopIteration:
                live.pop(t)
        exp = sorted(keys_all)[:m]
        assert L == exp + [EMPTY64] * (m - len(exp)), (trial, L, exp)


def _blobs(n=1500, d=6, k=5, seed=4):
    from mikmeans.data import blobs as B

    return B.make_blobs(n, d, k, seed=seed)


def _expect(X, C, m, dtype=torch.float32, farthest=False):
    idx, d2 = ref.topk(X.to(dtype), C, 1)
    return brute_force(idx, d2, C.shape[0], m, farthest=farthest)


def test_estimators_cluster_exemplars_cpu():
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    C = km.cluster_centers_
    for far in (False, True):
        rows, d2 = km.cluster_exemplars(X, 7, farthest=far, squared=True)
        assert torch.is_tensor(rows) and torch.is_tensor(d2)
        exp_rows, exp_d2 = _expect(X, C, 7, farthest=far)
        assert_lists(rows, d2, exp_rows, exp_d2)
        rows2, dist = km.cluster_exemplars(X, 7, farthest=far)
        assert torch.equal(rows2, rows) and torch.equal(dist, d2.sqrt())
        # every listed row is assigned to its cluster, at that distance
        lab = km.predict(X)
        for c in range(5):
            assert bool((lab[rows[c]] == c).all())
        torch.testing.assert_close(dist, (X[rows.flatten()] - C.repeat_interleave(7, 0)).norm(dim=1).view(5, 7),
                                   rtol=1e-4, atol=1e-4)
        # the lists do not depend on the row blocks; numpy in, numpy out
        b = km.cluster_exemplars(X, 7, farthest=far, squared=True, block_rows=77)
        assert torch.equal(b[0], rows) and torch.equal(b[1], d2)
        nr, nd = km.cluster_exemplars(X.numpy(), 7, farthest=far, squared=True)
        assert isinstance(nr, np.ndarray) and isinstance(nd, np.ndarray)
        assert_lists(nr, nd, exp_rows, exp_d2)
    # m counts rows, not centres: it may exceed K; a short cluster is padded with -1 / NaN
    rows, dist = km.cluster_exemplars(X[:40], 64)
    cnt = torch.bincount(km.predict(X[:40]).long(), minlength=5)
    assert rows.shape == (5, 64) and torch.equal((rows >= 0).sum(1), cnt.clamp_max(64))
    assert bool(dist[rows < 0].isnan().all()) and not bool(dist[rows >= 0].isnan().any())
    with pytest.raises(RuntimeError):
        mikmeans.KMeans(3, device="cpu").cluster_exemplars(X, 3)
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(X)
    rows, d2 = mb.cluster_exemplars(X, 3, squared=True)
    assert_lists(rows, d2, *_expect(X, mb.cluster_centers_, 3))


def test_m_limits_raise():
    X = _blobs(200)
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    assert ops.EXEMPLAR_MAX == 64
    for bad in (0, 65):
        with pytest.raises(ValueError):
            km.cluster_exemplars(X, bad)
        with pytest.raises(ValueError):
            mikmeans.cluster_exemplars(X, km.cluster_centers_, bad)
        with pytest.raises(ValueError):
            ref.exemplar_table(torch.zeros((1, 1), dtype=torch.int32), torch.zeros((1, 1)), 5, bad)
    assert km.cluster_exemplars(X, 64)[0].shape == (5, 64)


def test_cosine_model_lists_unit_rows():
    X = _blobs(800, 7, 4, seed=9)
    km = mikmeans.KMeans(4, metric="cosine", device="cpu", seed=0, max_iter=10).fit(X)
    from mikmeans.api import _unit_rows

    rows, d2 = km.cluster_exemplars(X * 3.0, 5, farthest=True, squared=True)
    Xu = _unit_rows(X * 3.0)
    assert_lists(rows, d2, *_expect(Xu, km.cluster_centers_, 5, farthest=True))
    dist = km.cluster_exemplars(X * 3.0, 5, farthest=True)[1]
    d = torch.cdist(Xu.double(), km.cluster_centers_.double())
    lab = d.argmin(1)
    for c in range(4):
        assert float(dist[c, 0]) == pytest.approx(float(d[lab == c, c].max()), rel=1e-4)
    assert float(dist.max()) <= 2.0 + 1e-6


def test_functional_cluster_exemplars():
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    C = km.cluster_centers_
    rows, dist = mikmeans.cluster_exemplars(X, C, 4)
    er, ed = km.cluster_exemplars(X, 4)
    assert torch.equal(rows, er) and torch.equal(dist, ed)
    fr, fd = mikmeans.cluster_exemplars(X.numpy(), C.numpy(), 4, farthest=True)
    er, ed = km.cluster_exemplars(X, 4, farthest=True)
    assert isinstance(fr, np.ndarray) and np.array_equal(fr, er.numpy()) and np.array_equal(fd, ed.numpy())
    br, bd = mikmeans.cluster_exemplars(X, C, 4, dtype="bfloat16")
    exp_rows, exp_d2 = _expect(X, C, 4, torch.bfloat16)
    assert np.array_equal(br.numpy(), exp_rows) and torch.equal(bd, torch.from_numpy(exp_d2).sqrt())
    assert "cluster_exemplars" in mikmeans.__all__


def test_farthest_is_the_reports_radius():
    """Cross-check against cluster_report: the farthest row's squared distance has the bit
    pattern of the report's maximum word, and a list holds min(m, count) rows."""
    X = _blobs(1500, 6, 5, seed=21)
    X[11] = INF
    km = mikmeans.KMeans(7, device="cpu", seed=0, max_iter=3).fit(_blobs(1500, 6, 5, seed=21))
    km.cluster_centers_[6] = 1e6                                          # an empty cluster
    rep = km.cluster_report(X)
    for m in (1, 3, 64):
        rows, d2 = km.cluster_exemplars(X, m, farthest=True, squared=True)
        full = rep.counts > 0
        assert int(full.sum()) >= 2 and not bool(full[6])
        assert torch.equal(d2[full, 0].view(torch.int32).long(), rep.table[full, 17])
        assert torch.equal((rows >= 0).sum(1), rep.counts.clamp_max(m))
        assert 11 not in rows.flatten().tolist()
        near, _ = km.cluster_exemplars(X, m)
        assert torch.equal((near >= 0).sum(1), rep.counts.clamp_max(m))


def test_cli_report_exemplars(tmp_path):
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    km.save(tmp_path / "m")
    np.save(tmp_path / "p.npy", X.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "mikmeans", "report", "--model", "m", "--input", "p.npy", "--device", "cpu"]
    plain = subprocess.run([*base, "--output", "plain.json"], cwd=tmp_path, env=env, capture_output=True, text=True,
                           timeout=300)
    assert plain.returncode == 0, plain.stderr
    exp = km.cluster_report(X).to_dict()
    # without the flag: today's file, byte for byte
    assert (tmp_path / "plain.json").read_text() == json.dumps(exp, indent=1)
    r = subprocess.run([*base, "--output", "ex.json", "--exemplars", "3"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads((tmp_path / "ex.json").read_text())
    rows, dist = km.cluster_exemplars(X, 3)
    assert got.pop("exemplars") == _jsonable({"m": 3, "farthest": False, "rows": rows, "distances": dist})
    assert got == exp
    assert r.stdout.strip().splitlines()[-1] == plain.stdout.strip().splitlines()[-1]       # the summary line
    # --farthest, and a cluster without rows: its padding (NaN) is written as null
    km.cluster_centers_[4] = 1e6
    km.save(tmp_path / "m")
    r = subprocess.run([*base, "--output", "far.json", "--exemplars", "2", "--farthest"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    ex = json.loads((tmp_path / "far.json").read_text())["exemplars"]
    rows, dist = km.cluster_exemplars(X, 2, farthest=True)
    assert ex == _jsonable({"m": 2, "farthest": True, "rows": rows, "distances": dist})
    assert ex["rows"][4] == [-1, -1] and ex["distances"][4] == [None, None] and ex["rows"][0][0] >= 0


WS_N, WS_K, WS_M = 2001, 6, 5


def _ws_exemplars(comm):
    X = _blobs(WS_N, 6, WS_K, seed=12)
    X[5] = INF                                                        # (a row no list holds)
    C = _blobs(WS_K, 6, WS_K, seed=13)
    C[3] = 1e6                                                        # (an empty cluster: padded)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    out = {}
    for far in (False, True):
        rows, dist = km.cluster_exemplars(X[s:e], WS_M, farthest=far)
        out[far] = (rows, dist)
    return out


def test_exemplars_are_world_size_invariant():
    from mikmeans.parallel import Comm

    one = _ws_exemplars(Comm.local())
    for far in (False, True):
        rows, dist = one[far]
        assert 5 not in rows.flatten().tolist() and bool((rows[3] == -1).all()) and bool(dist[3].isnan().all())
        assert int(rows.max()) > WS_N * 2 // 3                        # rows of the last shard are listed
    for world in (2, 3):
        for o in spawn_local(_ws_exemplars, world):
            for far in (False, True):
                assert torch.equal(o[far][0], one[far][0])
                assert torch.equal(o[far][1].view(torch.int32), one[far][1].view(torch.int32))   # (bits: NaN == NaN)


def test_exemplar_kernel_resources(tmp_path):
    """The built code object: exemplar_kernel<LDS> in both forms (global atomics, LDS-private)
    without scratch or spills."""
    from mikmeans import _build
    from mikmeans.utils import isa

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    assert "exemplars.hip" in _build.HIP_SOURCES
    src = _build.CSRC / "exemplars.hip"
    obj = _build._compile(src, _build.source_flags(src.name), verbose=False)
    res = [r for r in isa.kernel_resources(isa.device_elf(obj, tmp_path / "exemplars.dev.o"))
           if "exemplar_kernel<" in r.name]
    assert len(res) == 2, [r.name for r in res]
    bad = [(r.name, r.vgprs, r.vgpr_spills, r.scratch_bytes) for r in res if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
