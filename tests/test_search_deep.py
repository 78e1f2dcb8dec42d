"""search_deep on the CPU: the mirror against a brute-force stable sort, the radix select's mirrors
(ops.cpu.index_hist / index_select), padding, limits, the CLI, world-size invariance, the memory
plan and the register budget of the histogram kernel."""
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


def _fitted(n=600, d=6, K=7, **kw):
    X, _, Q = _ints(n, d, K)
    X, Q = torch.as_tensor(X), torch.as_tensor(Q)
    return X, Q, mikmeans.KMeans(K, device="cpu", seed=1, **kw).fit(X)


@pytest.fixture(scope="module")
def big():
    """3000 rows under 7 centres: m = 2048 is a real cut at nprobe = K."""
    X, C, Q = _ints(3000, 6, 7, nq=12, seed=3)
    Xt, Ct, Qt = torch.as_tensor(X), torch.as_tensor(C), torch.as_tensor(Q)
    return X, C, Q, Xt, Ct, Qt, ops.index_build(Xt, Ct)


@pytest.mark.parametrize("m,nprobe", [(1, 2), (32, 7), (33, 3), (100, 7), (2048, 7), (2048, 2)])
def test_mirror_against_brute_force(big, m, nprobe):
    X, C, Q, Xt, Ct, Qt, ix = big
    keys = ops.index_search_deep(ix, Qt, Ct, m, nprobe)
    assert keys.dtype == torch.int64 and keys.shape == (Q.shape[0], m)
    rows, d2 = ops.index_decode(keys)
    er, ed = _np_search(X, C, Q, m, nprobe)
    assert np.array_equal(rows.numpy(), er)
    assert np.array_equal(d2.numpy().astype(np.float64), ed, equal_nan=True)
    if m <= ops.INDEX_MAX_M:
        assert torch.equal(keys, ops.index_search(ix, Qt, Ct, m, nprobe))
    tie = d2[:, 1:] == d2[:, :-1]
    assert bool((rows[:, 1:][tie] > rows[:, :-1][tie]).all())          # equal distances: the lower row first


@pytest.mark.parametrize("m,nprobe", [(1, 1), (33, 3), (100, 7), (2048, 7), (2048, 1)])
def test_select_mirror_finds_the_mth_key(big, m, nprobe):
    """Four passes of index_hist / index_select: the prefix is the bit pattern of the m-th key (of
    the last one where the candidates are fewer), the rank its 0-based place among the rows that
    share it, and every pass's hits count the candidates under the pass's radius."""
    X, C, Q, Xt, Ct, Qt, ix = big
    nq = Q.shape[0]
    probes = ref.topk(Qt, Ct, nprobe)[0]
    bits, member, rid = ref.index_pair_bits(ix, Qt, probes)
    assert bits.shape == member.shape == (nq, 3000) and rid.shape == (3000,)
    lab = np.argmin(_np_d2(X, C), axis=1)
    assert np.array_equal(member.sum(1).numpy(), np.array([np.isin(lab, p).sum() for p in probes.numpy()]))
    srt = torch.where(member, bits, 1 << 40).sort(dim=1).values      # the candidates' bits ascending
    cand_e = member.sum(1)
    prefix = rank = cand = None
    for p in range(4):
        table = ref.index_hist(bits, member, prefix, p)
        assert table.shape == (nq, 256) and table.dtype == torch.int64
        prefix, rank, hits, cand = ref.index_select(table, prefix, rank, cand, m, p)
        assert prefix.dtype == torch.int32 and torch.equal(cand, cand_e)
        s = 24 - 8 * p
        radius = prefix.to(torch.int64) | ((1 << s) - 1)
        assert torch.equal(hits, (member & (bits <= radius[:, None])).sum(1))
        assert bool((hits >= cand.clamp(max=m)).all())
        if p == 0:
            assert torch.equal(table.sum(1), cand_e)
    found = cand_e.clamp(max=m)
    assert bool((found > 0).all())
    kth = srt.gather(1, (found - 1)[:, None])[:, 0]
    assert torch.equal(prefix.to(torch.int64), kth)
    below = (member & (bits < kth[:, None])).sum(1)
    assert torch.equal(rank, found - 1 - below)
    ties = (member & (bits == kth[:, None])).sum(1)
    assert torch.equal(hits, below + ties) and bool((ties > 1).any())   # ties at the m-th place: hits > m


def test_select_of_a_query_without_candidates_is_zero():
    table = torch.zeros((2, 256), dtype=torch.int64)
    table[1, 0x42] = 3
    prefix, rank, hits, cand = ref.index_select(table, None, None, None, 5, 0)
    assert prefix.tolist() == [0, 0x42 << 24] and rank.tolist() == [0, 2] and hits.tolist() == [0, 3]
    assert cand.tolist() == [0, 3]
    bits = torch.tensor([[0x42000001, 0x42000001, 0x42000100]] * 2)
    member = torch.tensor([[False] * 3, [True] * 3])
    for p in (1, 2, 3):
        prefix, rank, hits, cand = ref.index_select(ref.index_hist(bits, member, prefix, p), prefix, rank, cand, 5, p)
        assert prefix[0] == 0 and rank[0] == 0 and hits[0] == 0 and cand.tolist() == [0, 3]
    assert int(prefix[1]) == 0x42000100 and int(rank[1]) == 0 and int(hits[1]) == 3
    with pytest.raises(ValueError):
        ref.index_hist(bits, member, None, 1)
    with pytest.raises(ValueError):
        ref.index_hist(bits, member, prefix, 4)


def test_estimator_search_deep_cpu():
    X, Q, km = _fitted()
    K = km.n_clusters
    ix = km.build_index(X)
    rows, dist = ix.search_deep(Q, 100, nprobe=K)
    assert rows.shape == dist.shape == (40, 100) and rows.dtype == torch.int64 and dist.dtype == torch.float32
    er, ed = _np_search(X.numpy(), km.cluster_centers_.numpy(), Q.numpy(), 100, K)
    assert np.array_equal(rows.numpy(), er)
    _, sq = ix.search_deep(Q, 100, nprobe=K, squared=True)
    assert np.array_equal(sq.numpy().astype(np.float64), ed) and torch.equal(dist, sq.sqrt())
    for m in (1, 8, 32):                                              # up to the scan's length: search itself
        a, b = ix.search_deep(Q, m, nprobe=3), ix.search(Q, m, nprobe=3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    for passes in (1, 2, 3, 4):
        again = ix.search_deep(Q, 100, nprobe=K, passes=passes)
        assert torch.equal(again[0], rows) and torch.equal(again[1], dist)
    nr, nd = ix.search_deep(Q.numpy(), 100, nprobe=K)                 # numpy in, numpy out
    assert isinstance(nr, np.ndarray) and nr.dtype == np.int64 and nd.dtype == np.float32
    assert np.array_equal(nr, rows.numpy()) and np.array_equal(nd, dist.numpy())


def test_search_deep_pads_with_minus_one_and_nan():
    X, Q, km = _fitted()
    km.cluster_centers_[2] = 1e6                          # an empty cluster ...
    ix = km.build_index(X)
    far = torch.full((1, X.shape[1]), 1e6)                # ... and a query that probes only it
    rows, dist = ix.search_deep(torch.cat([far, Q]), 40, nprobe=1)
    assert rows[0].tolist() == [-1] * 40 and bool(dist[0].isnan().all())
    sizes = ix.list_sizes[km.predict_topk(Q, 1)[0][:, 0].long()].clamp(max=40)
    assert torch.equal((rows[1:] >= 0).sum(1), sizes) and torch.equal((~dist[1:].isnan()).sum(1), sizes)
    rows, dist = ix.search_deep(Q, 2048, nprobe=km.n_clusters)        # fewer candidates than m
    assert bool((rows[:, :600] >= 0).all()) and bool((rows[:, 600:] == -1).all()) and bool(dist[:, 600:].isnan().all())
    none = km.build_index(X[:0])                          # no rows at all
    rows, dist = none.search_deep(Q, 50, nprobe=3)
    assert rows.shape == (40, 50) and bool((rows == -1).all()) and bool(dist.isnan().all())


def test_limits_raise_and_search_keeps_its_bound():
    X, Q, km = _fitted()
    ix = km.build_index(X)
    assert ops.INDEX_DEEP_MAX_M == 2048 and ops.INDEX_DEEP_OVERSHOOT == 2 and ops.INDEX_MAX_M == 32
    for m, nprobe in ((0, 1), (2049, 1), (40, 0), (40, km.n_clusters + 1)):
        with pytest.raises(ValueError):
            ix.search_deep(Q, m, nprobe=nprobe)
        with pytest.raises(ValueError):
            ops.index_search_deep(ix._index, Q, km.cluster_centers_, m, nprobe)
    for passes in (0, 5):
        with pytest.raises(ValueError):
            ix.search_deep(Q, 40, nprobe=2, passes=passes)
    with pytest.raises(ValueError):
        ix.search_deep(Q[:, :3], 40)                      # another width
    with pytest.raises(ValueError):
        ix.search(Q, 33)                                  # search itself ends at 32
    with pytest.raises(ValueError):
        ops.index_search(ix._index, Q, km.cluster_centers_, 33, 2)


def test_cli_search_deep(tmp_path):
    X, Q, km = _fitted()
    km.save(tmp_path / "m")
    np.save(tmp_path / "x.npy", X.numpy())
    np.save(tmp_path / "q.npy", Q.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "mikmeans", "search", "--model", "m", "--input", "x.npy", "--queries", "q.npy",
            "--device", "cpu", "--nprobe", "3"]
    r = subprocess.run([*base, "--deep", "--top", "100", "--output", "out.npz"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows, dist = km.build_index(X).search_deep(Q, 100, nprobe=3)
    got = np.load(tmp_path / "out.npz")
    assert got["rows"].dtype == np.int64 and got["distances"].dtype == np.float32
    assert np.array_equal(got["rows"], rows.numpy()) and np.array_equal(got["distances"], dist.numpy(), equal_nan=True)
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"n_samples": 600, "n_queries": 40, "top": 100, "nprobe": 3,
                                                             "found": int((rows >= 0).sum())}
    r = subprocess.run([*base, "--top", "33", "--output", "no.npz"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "--top must be in [1, 32]" in r.stderr and not (tmp_path / "no.npz").exists()
    r = subprocess.run([*base, "--deep", "--top", "2049"], cwd=tmp_path, env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "--top must be in [1, 2048]" in r.stderr


WS_N, WS_K, WS_M = 1201, 6, 40


def _ws_search_deep(comm):
    X, C, Q = _ints(WS_N - 1, 6, WS_K, nq=50, seed=12)
    X = torch.as_tensor(np.concatenate([X, X[:1]]))
    X[5] = float("inf")                                               # (a row no list holds)
    C = torch.as_tensor(C)
    C[3] = 1e6                                                        # (an empty cluster)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    ix = km.build_index(X[s:e])
    return {nprobe: ix.search_deep(torch.as_tensor(Q), WS_M, nprobe=nprobe) for nprobe in (1, 2, WS_K)}


def test_search_deep_is_world_size_invariant():
    from mikmeans.parallel import Comm

    one = _ws_search_deep(Comm.local())
    rows, dist = one[WS_K]
    assert rows.shape == (50, WS_M) and 5 not in rows.flatten().tolist() and int(rows.max()) > WS_N * 2 // 3
    tie = dist[:, 1:] == dist[:, :-1]
    assert bool(tie.any()) and bool((rows[:, 1:][tie] > rows[:, :-1][tie]).all())
    for world in (2, 3):
        for o in spawn_local(_ws_search_deep, world):
            for nprobe in (1, 2, WS_K):
                assert torch.equal(o[nprobe][0], one[nprobe][0])
                assert torch.equal(o[nprobe][1].view(torch.int32), one[nprobe][1].view(torch.int32))   # (bits: NaN == NaN)


def test_plan_lists_the_deep_search_buffers():
    n, D, K, nq, m, nprobe = 20000, 30, 37, 5000, 100, 8
    plan = memplan.plan_index_search_deep(n, D, K, torch.bfloat16, nq=nq, m=m, nprobe=nprobe)
    assert plan.mode == "index-search-deep" and plan.fits and set(plan.transient) == {"select", "collect"}
    assert {"row_pack", "cn", "order", "offsets", "tile_offsets", "result_keys"} == set(plan.persistent)
    assert plan.persistent["result_keys"] == memplan._r(nq * m * 8)
    sel, col = plan.transient["select"], plan.transient["collect"]
    assert sel["histogram"] == memplan._r(nq * 1024) and {"prefix", "rank", "hits", "candidates", "pair_order", "item_cum"} <= set(sel)
    assert col["keys"] == memplan._r(ops.INDEX_DEEP_OVERSHOOT * m * nq * 8) and {"radius", "pair_counts", "pair_base"} <= set(col)
    # the blocks are the op's, and a block's table, pair arrays and keys stay within INDEX_SCAN_KEYS keys' worth
    for mm, pp in ((100, 8), (2048, 1024), (1, 1), (2048, 1)):
        B = memplan.deep_block_queries(mm, pp)
        assert B == ops.deep_block_queries(mm, pp) >= 1
        assert B * (1024 + 28 * pp + 8 * ops.INDEX_DEEP_OVERSHOOT * mm) <= 8 * ops.INDEX_SCAN_KEYS
    huge = memplan.plan_index_search_deep(n, D, K, torch.bfloat16, nq=1 << 30, m=2048, nprobe=nprobe)
    Bh = memplan.deep_block_queries(2048, nprobe)
    assert huge.transient["select"]["histogram"] == memplan._r(Bh * 1024)       # a block's, whatever nq
    huge.budget = 1 << 30
    assert not huge.fits                                             # (the result alone is 16 TiB)


def test_hist_kernels_register_budget(tmp_path):
    """Every histogram instantiation runs without scratch or spills and fits two waves per SIMD
    (<= 256 VGPRs) wherever the count pass of the same (T, DPAD, P) does; it is built for the
    count pass's widths."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    assert "deep.hip" in _build.HIP_SOURCES
    hist = _kernels("deep.hip", "ivf_hist_kernel", tmp_path)                 # (T, DPAD, P)
    count = {t[:3]: r for t, r in _kernels("range.hip", "ivf_range_kernel", tmp_path).items() if t[3] == "false"}
    assert {t[:2] for t in hist} == {t[:2] for t in count} and len(hist) >= 14
    assert {t[2] for t in hist} == {"1"}                                      # (one pair block a wave: csrc/deep.hip)
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes) for t, r in hist.items() if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
    over = [(t, r.vgprs) for t, r in hist.items() if r.vgprs > 256 and (t not in count or count[t].vgprs <= 256)]
    assert not over, over
