"""cluster_report on the CPU: the integer mirror of csrc/quality.hip against plain float64
NumPy, the decode, the estimators, the functional form, the CLI's ``report`` and world-size
invariance over gloo ranks (the GPU kernel against this mirror: test_gpu_quality.py)."""
import json
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref
from mikmeans.parallel import shard_range
from mikmeans.parallel.launch import spawn_local

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QW = ref.QUALITY_WORDS
INF, NAN = float("inf"), float("nan")


def words_int(row, lo):
    """The integer sum_j W[lo + j] * 2^(32 j) of one label's seven digit words: its sum at scale 2^-64."""
    return sum(int(row[lo + j]) << (32 * j) for j in range(7))


def synthetic(n, K, seed, m=2):
    """(idx, d2) as a top-2 result: every d2 a multiple of 2^-14 below 2^11 (so every sum of
    a^2 is exact in float64 and no addend is truncated at 2^-64), some rows at distance 0."""
    g = torch.Generator().manual_seed(seed)
    k0 = torch.randint(0, K, (n,), generator=g)
    k1 = (k0 + 1 + torch.randint(0, max(K - 1, 1), (n,), generator=g)) % K
    a2 = torch.randint(0, 1 << 24, (n,), generator=g).float() / (1 << 14)
    a2[::17] = 0.0
    b2 = a2 + torch.randint(0, 1 << 24, (n,), generator=g).float() / (1 << 14)
    b2[::34] = 0.0                                                        # (a^2 = b^2 = 0: duplicate centres)
    idx = torch.stack([k0, k1], 1).to(torch.int32)[:, :m].contiguous()
    return idx, torch.stack([a2, b2], 1)[:, :m].contiguous()


def hard_inputs():
    """{name: (idx, d2, K)}: the inputs that stress the digit words and the special cases."""
    out = {}
    # magnitudes mixed within one cluster: the sum carries across digit words
    vals = torch.tensor([2.0 ** -40, 1.0, 3.0e9, 2.0 ** 100, 0.0, 2.0 ** -40 * 3, 7.25, 2.0 ** 100], dtype=torch.float32)
    a2 = vals.repeat(40)
    out["mixed"] = (torch.tensor([[1, 2]], dtype=torch.int32).repeat(a2.numel(), 1).contiguous(),
                    torch.stack([a2, a2 * 4], 1).contiguous(), 3)
    # every row in one label, the other clusters empty
    idx, d2 = synthetic(700, 2, 5)
    idx[:, 0], idx[:, 1] = 2, 0
    out["one_label"] = (idx, d2, 4)
    # m = 1 (K = 1)
    idx, d2 = synthetic(300, 1, 6, m=1)
    out["k1"] = (idx, d2, 1)
    # b^2 = 0 on every row (duplicate centres), b^2 = +inf, and rows whose a^2 is not finite
    z = torch.zeros(64, 2)
    out["b_zero"] = (torch.tensor([[0, 1]], dtype=torch.int32).repeat(64, 1).contiguous(), z, 2)
    idx, d2 = synthetic(200, 3, 7)
    d2[::3, 1] = INF
    out["b_inf"] = (idx, d2, 3)
    idx, d2 = synthetic(400, 5, 8)
    d2[::5, 0], d2[::5, 1] = INF, INF
    d2[1::10, 0], d2[1::10, 1] = NAN, NAN
    d2[2::10, 1] = NAN                                                    # (a finite row with a NaN b^2: s = 0)
    out["nonfinite"] = (idx, d2, 5)
    return out


def check_against_numpy(table, idx, d2, K):
    """Every word of ``table`` against float64 NumPy / exact rational sums of the same rows."""
    T = table.cpu().numpy()
    k = idx[:, 0].cpu().numpy().astype(np.int64)
    d = d2.cpu().numpy().astype(np.float64)
    a2 = d[:, 0]
    fin = np.isfinite(a2)
    assert T.shape == (K, QW) and T.dtype == np.int64
    assert not T[:, 18:].any()
    for c in range(K):
        rows = (k == c) & fin
        nk = int(rows.sum())
        assert T[c, 7] == nk, (c, T[c, 7], nk)
        assert T[c, 15] == int(((k == c) & ~fin).sum())
        a2c = a2[rows]
        mx = np.float32(a2c.max()) if nk else np.float32(0)
        assert T[c, 17] == int(mx.view(np.uint32)), (c, T[c, 17])
        exact = sum((Fraction(float(v)) for v in a2c), Fraction(0)) * 2 ** 64
        assert exact.denominator == 1 and words_int(T[c], 0) == exact.numerator, c   # (no d2 in (0, 2^-40))
        suma = math.fsum(np.sqrt(a2c))
        got = words_int(T[c], 8) / 2.0 ** 64
        assert abs(got - suma) <= 1e-12 * suma + nk * 2.0 ** -60, (c, got, suma)
        if d.shape[1] == 2:
            b2 = d[rows, 1]
            with np.errstate(all="ignore"):
                s = np.clip(1.0 - np.sqrt(a2c / b2), 0.0, 1.0)
            s = np.where(np.isinf(b2), 1.0, s)
            s = np.where(b2 > 0, s, 0.0)
            assert abs(T[c, 16] / 2.0 ** 31 - math.fsum(s)) <= nk * 2.0 ** -30, (c, T[c, 16] / 2.0 ** 31, s.sum())
        else:
            assert T[c, 16] == 0


def test_mirror_matches_float64_numpy():
    for n, K, seed in ((1, 4, 0), (1000, 7, 1), (5000, 64, 2)):
        idx, d2 = synthetic(n, K, seed)
        T = ref.quality_table(idx, d2, K)
        check_against_numpy(T, idx, d2, K)
        # exactly the float64 sum, and the decode of the words is that sum too
        rep = ops.quality_decode(T, torch.zeros(K, 2))
        exp = np.zeros(K)
        np.add.at(exp, idx[:, 0].numpy(), d2[:, 0].double().numpy())
        assert np.array_equal(rep["cluster_inertia"].numpy(), exp)
        assert rep["inertia"] == float(exp.sum()) and rep["n_samples"] == n
        assert torch.equal(rep["counts"], torch.bincount(idx[:, 0].long(), minlength=K))


@pytest.mark.parametrize("name", sorted(hard_inputs()))
def test_mirror_hard_inputs(name):
    idx, d2, K = hard_inputs()[name]
    T = ref.quality_table(idx, d2, K)
    check_against_numpy(T, idx, d2, K)
    rep = ops.quality_decode(T, torch.zeros(K, 2))
    if name == "mixed":
        assert sum(1 for j in range(7) if T[1, j]) >= 4              # the sum spans the digit words
        assert rep["radius"][1] == 2.0 ** 50 and rep["counts"].tolist() == [0, 320, 0]
        # s = 1 - sqrt(1/4) on the 280 rows with a^2 > 0, s = 0 on the 40 rows with a^2 = b^2 = 0
        assert float(rep["cluster_silhouette"][1]) == pytest.approx(0.5 * 280 / 320, abs=1e-9)
    if name == "one_label":
        assert rep["counts"].tolist() == [0, 0, 700, 0] and not T[[0, 1, 3]].any()
        assert math.isnan(rep["davies_bouldin"]) and bool(rep["mean_distance"][[0, 1, 3]].isnan().all())
        assert rep["radius"][[0, 1, 3]].tolist() == [0, 0, 0]
    if name == "k1":
        assert math.isnan(rep["silhouette"]) and rep["counts"].tolist() == [300]
    if name == "b_zero":
        assert rep["silhouette"] == 0.0 and rep["inertia"] == 0.0 and rep["counts"].tolist() == [64, 0]
    if name == "b_inf":
        assert int(T[:, 16].sum()) >= 67 << 31                       # (67 rows with s = 1)
    if name == "nonfinite":
        assert int(T[:, 15].sum()) == 120 and rep["n_samples"] == 280
        assert int(rep["n_nonfinite"].sum()) == 120 and math.isfinite(rep["inertia"])


def test_table_is_order_and_split_free():
    idx, d2 = synthetic(3000, 11, 3)
    big = hard_inputs()["mixed"]
    idx, d2 = torch.cat([idx, big[0]]), torch.cat([d2, big[1]])
    T = ref.quality_table(idx, d2, 11)
    p = torch.randperm(idx.shape[0], generator=torch.Generator().manual_seed(0))
    assert torch.equal(ref.quality_table(idx[p], d2[p], 11), T)
    acc = torch.zeros((11, QW), dtype=torch.int64)
    ops.quality_accumulate(acc, idx[:1234], d2[:1234])
    ops.quality_accumulate(acc, idx[1234:], d2[1234:])
    assert torch.equal(acc, T)
    with pytest.raises(ValueError):
        ops.quality_accumulate(torch.zeros((11, 3), dtype=torch.int64), idx, d2)
    with pytest.raises(ValueError):
        ref.quality_table(idx, d2[:, :1], 11)


def test_davies_bouldin_hand_placed():
    """Five centres: 3 duplicates 1 (separation 0 counts as +inf, so that pair's ratio is 0)
    and 4 is empty; the S_k are the mean distances of hand-placed rows."""
    C = torch.tensor([[0.0, 0.0], [10.0, 0.0], [0.0, 10.0], [10.0, 0.0], [50.0, 50.0]])
    lab = [0] * 4 + [1] * 3 + [2] * 5 + [3] * 2
    a = np.array([1.0, 2.0, 3.0, 2.0, 4.0, 4.0, 1.0, 0.5, 0.5, 0.5, 0.5, 3.0, 6.0, 2.0])
    idx = torch.tensor([[k, (k + 1) % 5] for k in lab], dtype=torch.int32)
    d2 = torch.tensor(np.stack([a * a, a * a * 4], 1), dtype=torch.float32)
    rep = ops.quality_decode(ref.quality_table(idx, d2, 5), C)
    S = np.array([a[np.array(lab) == k].mean() for k in range(4)])
    assert np.allclose(rep["mean_distance"][:4].numpy(), S, rtol=1e-15) and math.isnan(rep["mean_distance"][4])
    Cn = C.double().numpy()[:4]
    worst = []
    for k in range(4):
        r = []
        for l in range(4):
            if l != k:
                sep = np.linalg.norm(Cn[k] - Cn[l])
                r.append((S[k] + S[l]) / sep if sep > 0 else 0.0)
        worst.append(max(r))
    assert rep["davies_bouldin"] == pytest.approx(np.mean(worst), rel=1e-14)
    assert rep["silhouette"] == pytest.approx(0.5, abs=1e-9)
    assert rep["balance"] == {"max": 5, "min": 0, "gap": 5, "ratio": math.inf}
    one = ops.quality_decode(ref.quality_table(idx[:4], d2[:4], 5), C)          # one non-empty cluster
    assert math.isnan(one["davies_bouldin"])


def _blobs(n=1500, d=6, k=5, seed=4):
    from mikmeans.data import blobs as B

    return B.make_blobs(n, d, k, seed=seed)


def _expect_report(X, C, dtype=torch.float32):
    idx, d2 = ref.topk(X.to(dtype), C, min(2, C.shape[0]))
    return ref.quality_table(idx, d2, C.shape[0])


def test_estimators_cluster_report_cpu():
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    rep = km.cluster_report(X)
    assert isinstance(rep, mikmeans.ClusterReport) and torch.is_tensor(rep.counts)
    assert torch.equal(rep.table, _expect_report(X, km.cluster_centers_))
    assert torch.equal(rep.counts, torch.bincount(km.predict(X).long(), minlength=5))
    assert rep.n_samples == 1500 and rep.inertia == pytest.approx(-km.score(X), rel=1e-6)
    d = torch.cdist(X.double(), km.cluster_centers_.double())
    lab = d.argmin(1)
    for k in range(5):
        dk = d[lab == k, k]
        assert float(rep.mean_distance[k]) == pytest.approx(float(dk.mean()), rel=1e-4)
        assert float(rep.radius[k]) == pytest.approx(float(dk.max()), rel=1e-4)
        assert float(rep.rms_distance[k]) == pytest.approx(float((dk * dk).mean().sqrt()), rel=1e-4)
    two = d.sort(dim=1).values[:, :2]
    assert rep.silhouette == pytest.approx(float((1 - two[:, 0] / two[:, 1]).mean()), rel=1e-4)
    assert 0 < rep.davies_bouldin < 5 and rep.balance["max"] == int(rep.counts.max())
    # the table does not depend on the row blocks
    assert torch.equal(km.cluster_report(X, block_rows=7).table, rep.table)
    # numpy in, numpy out; JSON round trip
    nrep = km.cluster_report(X.numpy())
    assert isinstance(nrep.counts, np.ndarray) and isinstance(nrep.table, np.ndarray)
    assert np.array_equal(nrep.table, rep.table.numpy()) and nrep.inertia == rep.inertia
    dd = rep.to_dict()
    assert json.loads(json.dumps(dd)) == dd and dd == nrep.to_dict()
    assert dd["clusters"]["counts"] == rep.counts.tolist() and dd["n_clusters"] == 5
    with pytest.raises(RuntimeError):
        mikmeans.KMeans(3, device="cpu").cluster_report(X)
    mb = mikmeans.MiniBatchKMeans(4, batch_size=64, max_iter=5, device="cpu", seed=0).fit(X)
    mrep = mb.cluster_report(X)
    assert torch.equal(mrep.table, _expect_report(X, mb.cluster_centers_))
    assert torch.equal(mrep.counts, torch.bincount(mb.predict(X).long(), minlength=4))


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_nonfinite_rows_are_left_out_of_every_fold(dtype):
    """Rows with a NaN or infinite coordinate (one NaN, a NaN in the last column, all +inf, one
    -inf, one 1e20 whose square overflows) through cluster_report, cluster_quantiles and
    cluster_exemplars on the mirrors: each equals the call on the finite subset X[keep], row ids
    mapped back, and the report counts the rows it left out.  (The kernels under the same
    contract: test_gpu_nonfinite.py; build_index: test_ivf.py.)"""
    g = torch.Generator().manual_seed(6)
    n, d, K = 513, 30, 37
    C = 8.0 * torch.randn(K, d, generator=g)
    X = (C[(torch.arange(n) % K)[torch.randperm(n, generator=g)]] + 0.25 * torch.randn(n, d, generator=g))
    X = X.to(getattr(torch, dtype)).float()
    bad = [0, 15, 16, 277, n - 1]
    X[0, 3], X[15, d - 1], X[16], X[277, 5], X[n - 1, 7] = NAN, NAN, INF, -INF, 1e20
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad] = False
    ids = keep.nonzero().flatten()
    km = mikmeans.KMeans(K, device="cpu", dtype=dtype)
    km.cluster_centers_ = C

    def bits(t):
        t = torch.as_tensor(t)
        return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32) if t.is_floating_point() else t

    def folds(Z, **kw):
        rep = km.cluster_report(Z, **kw)
        out = {k: getattr(rep, k) for k in ("counts", "cluster_inertia", "radius", "cluster_silhouette", "table")}
        out["left_out"] = int(rep.n_nonfinite.sum())
        out["q"], out["qn"] = km.cluster_quantiles(Z, (0, 0.5, 1), **kw)
        out["near"], out["near_d"] = km.cluster_exemplars(Z, 4, **kw)
        out["far"], out["far_d"] = km.cluster_exemplars(Z, 4, farthest=True, **kw)
        return out

    got, sub = folds(X), folds(X[keep])
    assert got.pop("left_out") == len(bad) and sub.pop("left_out") == 0
    assert int(got["counts"].sum()) == n - len(bad) and int(got["counts"].min()) > 0
    words = torch.arange(QW) != 15
    assert torch.equal(got.pop("table")[:, words], sub.pop("table")[:, words])
    for side in ("near", "far"):
        rows = sub.pop(side)
        assert torch.equal(got.pop(side), torch.where(rows < 0, rows, ids[rows.clamp_min(0)])), side
    for name, t in got.items():
        assert torch.equal(bits(t), bits(sub[name])), name
    assert bool(torch.isfinite(got["q"]).all()) and torch.equal(got["qn"], got["counts"])
    # any blocking, and NumPy in / NumPy out: the same answers
    again, host = folds(X, block_rows=77), folds(X.numpy())
    ref_ = folds(X)
    for name, t in ref_.items():
        if name != "left_out":
            assert torch.equal(bits(again[name]), bits(t)) and torch.equal(bits(host[name]), bits(t)), name
    assert again["left_out"] == host["left_out"] == len(bad)


def test_cosine_model_reports_on_unit_rows():
    X = _blobs(800, 7, 4, seed=9)
    km = mikmeans.KMeans(4, metric="cosine", device="cpu", seed=0, max_iter=10).fit(X)
    rep = km.cluster_report(X * 3.0)                                  # the scale of a row does not matter
    Xu = X / X.norm(dim=1, keepdim=True)
    assert torch.equal(rep.counts, torch.bincount(km.predict(X).long(), minlength=4))
    assert float(rep.radius.max()) <= 2.0 + 1e-6
    d = torch.cdist(Xu.double(), km.cluster_centers_.double()).min(1).values
    assert rep.inertia == pytest.approx(float((d * d).sum()), rel=1e-4)


def test_functional_cluster_report():
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    C = km.cluster_centers_
    rep = mikmeans.cluster_report(X, C)
    assert torch.equal(rep.table, km.cluster_report(X).table) and rep.davies_bouldin == km.cluster_report(X).davies_bouldin
    nrep = mikmeans.cluster_report(X.numpy(), C.numpy())
    assert isinstance(nrep.counts, np.ndarray) and np.array_equal(nrep.table, rep.table.numpy())
    b = mikmeans.cluster_report(X, C, dtype="bfloat16")
    assert torch.equal(b.table, _expect_report(X, C, torch.bfloat16))
    assert "cluster_report" in mikmeans.__all__


def test_cli_report(tmp_path):
    X = _blobs()
    km = mikmeans.KMeans(5, device="cpu", seed=0).fit(X)
    km.save(tmp_path / "m")
    np.save(tmp_path / "p.npy", X.numpy())
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "mikmeans", "report", "--model", "m", "--input", "p.npy",
                        "--output", "report.json", "--device", "cpu"], cwd=tmp_path, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    exp = km.cluster_report(X).to_dict()
    assert json.loads((tmp_path / "report.json").read_text()) == exp
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line == {k: exp[k] for k in ("n_samples", "inertia", "silhouette", "davies_bouldin", "balance")}


WS_N, WS_K = 2001, 6


def _ws_report(comm):
    X = _blobs(WS_N, 6, WS_K, seed=12)
    X[5] = INF                                                        # (a row no cluster counts)
    C = _blobs(WS_K, 6, WS_K, seed=13)
    s, e = shard_range(WS_N, comm.rank, comm.world)
    km = mikmeans.KMeans(WS_K, device="cpu", comm=comm)
    km.cluster_centers_ = C
    rep = km.cluster_report(X[s:e])
    return {"table": rep.table, "dict": json.dumps(rep.to_dict()), "mean": rep.mean_distance}


def test_report_is_world_size_invariant():
    from mikmeans.parallel import Comm

    one = _ws_report(Comm.local())
    assert int(one["table"][:, 15].sum()) == 1 and int(one["table"][:, 7].sum()) == WS_N - 1
    for world in (2, 3):
        for o in spawn_local(_ws_report, world):
            assert torch.equal(o["table"], one["table"])
            assert o["dict"] == one["dict"]
            assert torch.equal(o["mean"].view(torch.int64), one["mean"].view(torch.int64))   # (bits: NaN == NaN)


def test_quality_kernel_resources(tmp_path):
    """The built code object: quality_kernel<M, LDS> in both forms (global atomics, LDS-private),
    each for m = 1 and 2, without scratch or spills."""
    from mikmeans import _build
    from mikmeans.utils import isa

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    assert "quality.hip" in _build.HIP_SOURCES
    src = _build.CSRC / "quality.hip"
    obj = _build._compile(src, _build.source_flags(src.name), verbose=False)
    res = [r for r in isa.kernel_resources(isa.device_elf(obj, tmp_path / "quality.dev.o"))
           if "quality_kernel<" in r.name]
    assert len(res) == 4, [r.name for r in res]
    bad = [(r.name, r.vgprs, r.vgpr_spills, r.scratch_bytes) for r in res if r.vgpr_spills or r.scratch_bytes]
    assert not bad, bad
