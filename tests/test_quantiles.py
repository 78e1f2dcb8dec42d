"""cluster_quantiles on the CPU: the integer mirror of csrc/quantiles.hip (four radix-select
passes) against sorting every cluster, split and order freedom of the histograms, the estimators,
the functional form, the CLI's ``report --quantiles`` and world-size invariance over gloo ranks
(the GPU kernels against this mirror: test_gpu_quantiles.py)."""
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
from tests.test_gpu_exemplars import _synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
QS = (0.0, 0.1, 0.5, 0.9, 0.99, 1.0)
# (n, K, kind): one row; a ragged wave; distances from {0, 1, 2, 4} only; -0, +0, NaN, +-inf,
# negative distances and labels -1, K and 2^31 - 1
SHAPES = [(1, 3, "random"), (63, 3, "random"), (5000, 7, "ties"), (20_000, 37, "hard")]


def brute_force(idx, d2, K, qs):
    """(values float32 [K, Q], counts int64 [K]) by sorting every cluster's a^2 and indexing
    r = clamp(ceil(q * n_k) - 1, 0, n_k - 1), the product one float64 multiply."""
    k = idx[:, 0].cpu().numpy().astype(np.int64)
    d = d2[:, 0].cpu().numpy().astype(np.float32)
    vals = np.full((K, len(qs)), np.nan, dtype=np.float32)
    counts = np.zeros(K, dtype=np.int64)
    for c in range(K):
        a2 = np.sort(np.maximum(d[(k == c) & np.isfinite(d)], np.float32(0)) + np.float32(0))   # (-0 -> +0)
        n = counts[c] = len(a2)
        for j, q in enumerate(qs):
            if n:
                r = int(np.ceil(np.float64(q) * np.float64(n))) - 1
                vals[c, j] = a2[min(max(r, 0), n - 1)]
    return vals, counts


def mirror_passes(idx, d2, K, qs):
    """The four passes by ops.cpu alone: ``(tables, prefix, rank, counts)``."""
    q = torch.tensor(qs, dtype=torch.float64)
    prefix, rank, counts = ops.quantile_state(K, len(qs))
    tables = []
    for p in range(4):
        tables.append(ref.quantile_hist(idx, d2, K, prefix, p))
        prefix, rank, n = ref.quantile_select(tables[-1], q, prefix, rank, p)
        counts = n if p == 0 else counts
    return tables, prefix, rank, counts


def assert_values(values, counts, exp_values, exp_counts):
    """Counts equal, values equal as bit patterns (NaN for the empty clusters)."""
    values = np.asarray(values.cpu() if torch.is_tensor(values) else values)
    counts = np.asarray(counts.cpu() if torch.is_tensor(counts) else counts)
    assert values.dtype == np.float32 and counts.dtype == np.int64 and values.shape == exp_values.shape
    assert np.array_equal(counts, exp_counts), np.argwhere(counts != exp_counts)[:8]
    assert np.array_equal(values.view(np.int32), exp_values.view(np.int32)), \
        np.argwhere(values.view(np.int32) != exp_values.view(np.int32))[:8]


@pytest.mark.parametrize("n,K,kind", SHAPES)
def test_mirror_against_brute_force(n, K, kind):
    idx, d2 = _synthetic(n, K, kind)
    exp_values, exp_counts = brute_force(idx, d2, K, QS)
    tables, prefix, rank, counts = mirror_passes(idx, d2, K, QS)
    assert tables[0].shape == (K, 256) and all(t.shape == (K, len(QS), 256) and t.dtype == torch.int64 for t in tables[1:])
    assert prefix.dtype == torch.int32 and rank.dtype == torch.int64
    values = torch.where((counts > 0)[:, None], prefix.view(torch.float32), NAN)
    assert_values(values, counts, exp_values, exp_counts)
    # after the last pass the rank left is the position among equal values; every pass's bins of
    # a pair hold more rows than its rank
    full = counts > 0
    assert bool((rank[full] >= 0).all()) and bool((tables[3].sum(-1)[full] > rank[full]).all())
    # the driver, and the empty clusters: NaN and count 0
    v, c = ops.quantile_passes([(idx, d2)], K, QS)
    assert_values(v, c, exp_values, exp_counts)
    empty = exp_counts == 0
    assert bool(np.isnan(v.numpy()[empty]).all()) and not np.isnan(v.numpy()[~empty]).any()
    assert not np.signbit(v.numpy()[~empty]).any()                         # -0 counted as +0
    if n == 1:
        assert int(empty.sum()) == 2 and int(c.sum()) == 1
    if kind == "hard":
        assert int(c.sum()) < n and bool((v[:, 0] == 0).all())              # the -0 / +0 / clamped rows come first
    # q = 0 and q = 1 are the extremes; the quantiles ascend
    vn = v.numpy()[~empty]
    assert bool((np.diff(vn, axis=1) >= 0).all())
    try:
        for cl in np.nonzero(~empty)[0][:5]:
            sel = (idx[:, 0].numpy() == cl) & np.isfinite(d2[:, 0].numpy())
            a2 = np.maximum(d2[:, 0].numpy()[sel], np.float32(0))
            assert np.array_equal(np.quantile(a2, QS, method="inverted_cdf").astype(np.float32), v.numpy()[cl])
    except TypeError:                                                      # (a NumPy without the method)
        pass


def test_tables_are_split_and_order_free():
    n, K = 20_000, 37
    idx, d2 = _synthetic(n, K, "hard")
    tables, prefix, rank, counts = mirror_passes(idx, d2, K, QS)
    q = torch.tensor(QS, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    perm = torch.randperm(n, generator=g)
    starts = list(range(0, n, 777))
    for ix, dd, order in ((idx, d2, starts), (idx, d2, starts[::-1]), (idx[perm], d2[perm], starts)):
        P, R, C = ops.quantile_state(K, len(QS))
        for p in range(4):
            acc = None
            for s in order:
                acc = ops.quantile_hist(ix[s : s + 777], dd[s : s + 777], K, P, p, table=acc)
            assert torch.equal(acc, tables[p])
            ops.quantile_select(acc, q, P, R, C, p)
        assert torch.equal(P, prefix) and torch.equal(R, rank) and torch.equal(C, counts)
    # two halves summed the way a two-rank job's all-reduce sums them
    P, R, C = ops.quantile_state(K, len(QS))
    for p in range(4):
        t = ops.quantile_hist(idx[:9000], d2[:9000], K, P, p) + ops.quantile_hist(idx[9000:], d2[9000:], K, P, p)
        assert torch.equal(t, tables[p])
        ops.quantile_select(t, q, P, R, C, p)
    assert torch.equal(P, prefix)
    # column 0 is read through the row stride of a top-2 result
    wide = torch.stack([idx[:, 0], idx[:, 0] + 1], 1).contiguous(), torch.stack([d2[:, 0], d2[:, 0] + 1], 1).contiguous()
    assert torch.equal(ref.quantile_hist(*wide, K, None, 0), tables[0])
    with pytest.raises(ValueError):
        ref.quantile_hist(idx, d2, K, None, 4)
    with pytest.raises(ValueError):
        ref.quantile_hist(idx, d2, K, None, 1)
    with pytest.raises(ValueError):
        ref.quantile_hist(idx, d2[:, :0], K, None, 0)
    with pytest.raises(ValueError):
        ops.quantile_hist(idx, d2, K, prefix, 0, table=torch.zeros((K, 255), dtype=torch.int64))


def _blobs(n=1500, d=6, k=5, seed=4):
    from mikmeans.data import blobs as B

    return B.make_blobs(n, d, k, seed=seed)


def test_estimators_cluster_quantiles_cpu():
    X = _blobs(1500, 6, 5, seed=21)
    km = mikmeans.KMeans(7, device="cpu", seed=0, max_iter=3).fit(X)
    X[11] = INF                                                           # (a row that counts nowhere)
    km.cluster_centers_[6] = 1e6                                          # an empty cluster
    C = km.cluster_centers_
    assert ops.QUANTILE_MAX_Q == ref.QUANTILE_MAX_Q == 8 and ref.QUANTILE_BINS == 256
    v2, counts = km.cluster_quantiles(X, QS, squared=True)
    assert torch.is_tensor(v2) and v2.shape == (7, len(QS)) and v2.dtype == torch.float32 and counts.dtype == torch.int64
    idx, d2 = ref.topk(X, C, 1)
    assert_values(v2, counts, *brute_force(idx, d2, 7, QS))
    rep = km.cluster_report(X)
    full = rep.counts > 0
    assert int(full.sum()) >= 2 and not bool(full[6]) and bool(v2[6].isnan().all()) and int(counts[6]) == 0
    assert torch.equal(counts, rep.counts) and int(counts.sum()) == 1499
    # q = 1 is the report's radius word, q = 0 the nearest exemplar
    assert torch.equal(v2[full, -1].view(torch.int32).long(), rep.table[full, 17])
    near = km.cluster_exemplars(X, 1, squared=True)[1]
    assert torch.equal(v2[:, 0].view(torch.int32), near[:, 0].view(torch.int32))
    # Euclidean by default; the defaults; a scalar q; the row blocks; numpy in, numpy out
    v, c1 = km.cluster_quantiles(X, QS)
    assert torch.equal(c1, counts) and torch.equal(v.view(torch.int32), v2.sqrt().view(torch.int32))
    d3 = km.cluster_quantiles(X)[0]
    assert d3.shape == (7, 3) and torch.equal(d3[:, 0].view(torch.int32), v[:, 2].view(torch.int32))
    s, cs = km.cluster_quantiles(X, 0.5)
    assert s.shape == (7, 1) and torch.equal(s[:, 0].view(torch.int32), v[:, 2].view(torch.int32)) and torch.equal(cs, counts)
    b = km.cluster_quantiles(X, QS, squared=True, block_rows=77)
    assert torch.equal(b[0].view(torch.int32), v2.view(torch.int32)) and torch.equal(b[1], counts)
    nv, nc = km.cluster_quantiles(X.numpy(), np.asarray(QS), squared=True)
    assert isinstance(nv, np.ndarray) and isinstance(nc, np.ndarray)
    assert_values(nv, nc, v2.numpy(), counts.numpy())
    # the functional form
    fv, fc = mikmeans.cluster_quantiles(X, C, QS)
    assert torch.equal(fv.view(torch.int32), v.view(torch.int32)) and torch.equal(fc, counts)
    gv, gc = mikmeans.cluster_quantiles(X.numpy(), C.numpy(), 0.9)
    assert isinstance(gv, np.ndarray) and np.array_equal(gv[:, 0].view(np.int32), v[:, 3].numpy().view(np.int32))
    bv, bc = mikmeans.cluster_quantiles(X, C, QS, dtype="bfloat16")
    ib, db = ref.topk(X.to(torch.bfloat16), C, 1)
    eb = brute_force(ib, db, 7, QS)
    assert_values(bv, bc, torch.from_numpy(eb[0]).sqrt().numpy(), eb[1])
    assert "cluster_quantiles" in mikmeans.__all__
    with pytest.raises(RuntimeError):
        mikmeans.KMeans(3, device="cpu").cluster_quantiles(X, 0.5)
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(_blobs())
    mv, mc = mb.cluster_quantiles(_blobs(), QS, squared=True)
    assert_values(mv, mc, *brute_force(*ref.topk(_blobs(), mb.cluster_centers_, 1), 4, QS))


def test_q_limits_raise():
    X = _blobs(200)
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    for bad in ([0.1] * 9, [], 1.5, [0.5, -0.01], NAN, [0.5, NAN], INF, "half"):
        with pytest.raises(ValueError):
            km.cluster_quantiles(X, bad)
        with pytest.raises(ValueError):
            mikmeans.cluster_quantiles(X, km.cluster_centers_, bad)
        with pytest.raises(ValueError):
            ops.cluster_quantiles(X, km.cluster_centers_, bad)
    assert km.cluster_quantiles(X, [0.1] * 8)[0].shape == (5, 8)
    assert km.cluster_quantiles(X, [0.0, 1.0])[0].shape == (5, 2)


def test_cosine_model_takes_unit_rows():
    X = _blobs(800, 7, 4, seed=9)
    km = mikmeans.KMeans(4, metric="cosine", device="cpu", seed=0, max_iter=10).fit(X)
    from mikmeans.api import _unit_rows

    v2, counts = km.cluster_quantiles(X * 3.0, QS, squared=True)
    idx, d2 = ref.topk(_unit_rows(X * 3.0), km.cluster_centers_, 1)
    assert_values(v2, counts, *brute_force(idx, d2, 4, QS))
    assert float(v2.max()) <= 4.0 + 1e-5 and int(counts.sum()) == 800


def test_cli_report_quantiles(tmp_path):
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    km.cluster_centers_[4] = 1e6                                          # a cluster without rows: null
    km.save(tmp_path / "m")
    np.save(tmp_path / "p.npy", X.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    base = [sys.executable, "-m", "mikmeans", "report", "--model", "m", "--input", "p.npy", "--device", "cpu"]
    r = subprocess.run([*base, "--output", "q.json", "--quantiles", "0.5,0.9,0.99"], cwd=tmp_path, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = json.loads((tmp_path / "q.json").read_text())
    dist, counts = km.cluster_quantiles(X, (0.5, 0.9, 0.99))
    assert got.pop("quantiles") == _jsonable({"q": [0.5, 0.9, 0.99], "distances": dist, "counts": counts})
    assert got == km.cluster_report(X).to_dict()
    assert _jsonable(dist)[4] == [None, None, None] and int(counts[4]) == 0 and _jsonable(dist)[0][0] > 0
    for bad in ("0.5,x", "1.5", "", "0.1,0.1,0.1,0.1,0.1,0.1,0.1,0.1,0.1", "nan"):
        r = subprocess.run([*base, "--output", "bad.json", "--quantiles", bad], cwd=tmp_path, env=env,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--quantiles" in r.stderr and not (tmp_path / "bad.json").exists(), (bad, r.stderr)


WS_N, WS_K = 2001, 6


def _ws_quantiles(comm):
    X = _blobs(WS_N, 6, WS_K, seed=12)
    X[5] = INF                                                        # (a row that counts nowhere)
    C = _blobs(WS_K, 6, WS_K, seed=13)
    C[3] = 1e6                                                        # (an empty cluster: NaN)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    return km.cluster_quantiles(X[s:e], QS)


def test_quantiles_are_world_size_invariant():
    from mikmeans.parallel import Comm

    v, c = _ws_quantiles(Comm.local())
    assert int(c.sum()) == WS_N - 1 and int(c[3]) == 0 and bool(v[3].isnan().all()) and int((c > 0).sum()) >= 3
    for world in (2, 3):
        for ov, oc in spawn_local(_ws_quantiles, world):
            assert torch.equal(oc, c)
            assert torch.equal(ov.view(torch.int32), v.view(torch.int32))     # (bits: NaN == NaN)


def test_quantile_kernel_resources(tmp_path):
    """The built code object: the two histogram kernels (global atomics, LDS-private) and the
    select kernel, without scratch or spills."""
    from mikmeans import _build
    from mikmeans.utils import isa

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    assert "quantiles.hip" in _build.HIP_SOURCES
    src = _build.CSRC / "quantiles.hip"
    obj = _build._compile(src, _build.source_flags(src.name), verbose=False)
    res = [r for r in isa.kernel_resources(isa.device_elf(obj, tmp_path / "quantiles.dev.o"))
           if "quantile_" in r.name and "_kernel" in r.name]
    names = sorted(r.name.split("(")[0].split("::")[-1] for r in res)
    assert names == ["quantile_hist_kernel", "quantile_hist_lds_kernel", "quantile_select_kernel"], names
    bad = [(r.name, r.vgprs, r.vgpr_spills, r.scratch_bytes) for r in res if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
