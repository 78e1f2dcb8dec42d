"""The refined PQ search on CPU tensors: the re-rank mirror against a per-pair loop of the definition
and against float64, the shortlist against a brute-force rendering of the group rule, exactness on
integer data, the public interface, the command line, the memory plan, the launch planning of
csrc/rerankplan.h under ASan + UBSan and the registers of the built gfx950 kernel.  Every comparison
is bitwise unless stated otherwise."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = cpu.IVF_EMPTY_KEY
f32 = np.float32


# ---------------------------------------------------------------- the re-rank mirror
def _loop_d2(q, x, V):
    """The definition, one float32 operation at a time: q, x float32 numpy rows of F columns."""
    F = q.shape[0]
    pieces = (F + V - 1) // V
    a = [f32(0.0)] * 16
    for s in range(16):
        for t in range(s, pieces, 16):
            for e in range(V):
                c = t * V + e
                qv, xv = (q[c], x[c]) if c < F else (f32(0.0), f32(0.0))
                d = f32(qv - xv)
                p = f32(d * d)
                a[s] = f32(a[s] + p)
    h = [f32(f32(f32(a[o] + a[o + 1]) + f32(a[o + 2] + a[o + 3])) + f32(f32(a[o + 4] + a[o + 5]) + f32(a[o + 6] + a[o + 7])))
         for o in (0, 8)]
    return f32(h[0] + h[1])


def _loop_keys(Q, X, cand):
    V = 8 if Q.dtype == torch.bfloat16 else 4
    Qn, Xn = Q.float().numpy(), X.float().numpy()
    out = torch.full(cand.shape, EMPTY, dtype=torch.int64)
    with np.errstate(all="ignore"):
        for i in range(cand.shape[0]):
            for j in range(cand.shape[1]):
                r = int(cand[i, j])
                if 0 <= r < X.shape[0]:
                    d2 = _loop_d2(Qn[i], Xn[r], V)
                    bits = 0x7FC00000 if np.isnan(d2) else int(np.array(d2, dtype=f32).view(np.int32))
                    out[i, j] = (bits << 32) | r
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("F", [1, 8, 20, 70, 136])
def test_mirror_equals_the_plain_loop_and_is_close_to_float64(dtype, F):
    g = torch.Generator().manual_seed(F)
    n, nq, R = 9, 3, 5
    X = (torch.randn(n, F, generator=g) * 3).to(dtype)
    Q = (torch.randn(nq, F, generator=g) * 3).to(dtype)
    cand = torch.randint(0, n, (nq, R), generator=g)
    cand[0, 1], cand[1, 0], cand[2, 2], cand[2, 3] = -1, n, cand[2, 1], n + 5        # empty slots and a duplicate
    keys = cpu.rerank_keys(Q, X, cand)
    assert torch.equal(keys, _loop_keys(Q, X, cand))
    ok = (cand >= 0) & (cand < n)
    assert torch.equal(keys == EMPTY, ~ok)
    assert torch.equal(keys[ok] & 0xFFFFFFFF, cand[ok])
    assert int(keys[2, 2]) == int(keys[2, 1])                                        # the duplicate: its key twice
    # one rounding each for the subtract, the multiply and every add on the longest chain
    d2 = (keys[ok] >> 32).to(torch.int32).view(torch.float32).double()
    ref = ((Q.double()[:, None, :] - X.double()[cand.clamp(0, n - 1)]) ** 2).sum(-1)[ok]
    assert bool(((d2 - ref).abs() <= (F / 16 + 8) * 2.0 ** -24 * ref).all())
    # the m smallest, ascending, padded
    top = ops.rerank(Q, X, cand, 7)
    assert top.shape == (nq, 7) and torch.equal(top[:, :R], keys.sort(dim=1).values) and bool((top[:, R:] == EMPTY).all())
    assert torch.equal(ops.rerank(Q, X, cand, 2), keys.sort(dim=1).values[:, :2])


def test_mirror_non_finite_rows_and_strided_rows():
    g = torch.Generator().manual_seed(3)
    W = torch.randn(6, 40, generator=g)
    X = W[:, 3:27]                                                                   # a column slice
    X2 = X.contiguous()
    Q = torch.randn(2, 24, generator=g)
    cand = torch.arange(6)[None, :].expand(2, 6).contiguous()
    assert torch.equal(cpu.rerank_keys(Q, X, cand), cpu.rerank_keys(Q, X2, cand))
    X2[1, 5], X2[4, 0] = float("nan"), float("inf")
    keys = ops.rerank(Q, X2, torch.cat([cand, torch.full((2, 1), -1)], dim=1), 7)
    rows, d2 = ops.index_decode(keys)
    assert rows[:, 4:].tolist() == [[4, 1, -1]] * 2                                  # finite < inf < NaN < padding
    assert bool(torch.isinf(d2[:, 4]).all()) and bool((keys[:, 5] >> 32 == 0x7FC00000).all())


def test_rerank_errors():
    Q, X = torch.zeros(2, 8), torch.zeros(5, 8)
    cand = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(ValueError, match="one dtype"):
        ops.rerank(Q, X.to(torch.bfloat16), cand, 1)
    with pytest.raises(ValueError, match=r"Q \[nq, F\]"):
        ops.rerank(Q, X[:, :4], cand, 1)
    with pytest.raises(ValueError, match="candidates"):
        ops.rerank(Q, X, cand[:1], 1)
    with pytest.raises(ValueError, match="candidates"):
        ops.rerank(Q, X, cand.to(torch.int32), 1)
    with pytest.raises(ValueError, match="m >= 1"):
        ops.rerank(Q, X, cand, 0)


# ---------------------------------------------------------------- the shortlist
SK, SF, SM = 4, 16, 8
SSIZES = [2100, 0, 200, 37]                        # longer than 8 x 256 rows; shorter than 256; empty


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def lists(request):
    dtype = request.param
    g = torch.Generator().manual_seed(11)
    C = torch.randn(SK, SF, generator=g) * 12
    lab = torch.repeat_interleave(torch.arange(SK), torch.tensor(SSIZES))
    X = C[lab] + torch.randn(lab.numel(), SF, generator=g)
    X[5:25] = X[4]                                                                   # twenty copies: ties by row id
    X = X[torch.randperm(X.shape[0], generator=g)].to(dtype)
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    R = (X.float() - C[lab]).to(dtype).float()
    books = R[torch.randperm(X.shape[0], generator=g)[:256]].view(256, SM, SF // SM).permute(1, 0, 2).contiguous()
    index = ops.pq_build(X, C, SM, codebooks=books)
    assert (index.offsets[1:] - index.offsets[:-1]).tolist() == SSIZES
    Q = torch.cat([X[torch.randperm(X.shape[0], generator=g)[:9]].float() + 0.05, C[1:2] + 0.05]).to(dtype)
    return dtype, C, X, index, Q


def _brute_shortlist(index, C, Q, S, nprobe, dtype):
    """The group rule one pair at a time; the tables are those of the whole batch of queries."""
    G, s = (1, S) if S <= 32 else (S // 32, 32)
    nq, M = Q.shape[0], index.M
    probes = ops.topk(Q, C, nprobe)[0].long()
    RQ = (Q.float()[:, None, :] - C[probes]).to(dtype).view(nq * nprobe, SF)
    luts = ops.pq_lut(RQ, index.codebooks)
    out = torch.full((nq, nprobe, G, s), -1, dtype=torch.int64)
    for q in range(nq):
        for j in range(nprobe):
            l = int(probes[q, j])
            a, b = int(index.offsets[l]), int(index.offsets[l + 1])
            lut = luts[q * nprobe + j]
            c = index.codes[a:b].long()
            if a == b:
                continue
            acc = lut[0][c[:, 0]]
            for t in range(1, M):
                acc = torch.add(acc, lut[t][c[:, t]])
            bits = acc.view(torch.int32).tolist()
            rows = index.order[a:b].tolist()
            for grp in range(G):
                mine = sorted((bits[p], rows[p]) for p in range(b - a) if (p // 256) % G == grp)[:s]
                out[q, j, grp, : len(mine)] = torch.tensor([r for _, r in mine], dtype=torch.int64)
    return out.view(nq, nprobe * S)


@pytest.mark.parametrize("S", [1, 32, 64, 256])
def test_shortlist_equals_the_group_rule(lists, S):
    dtype, C, X, index, Q = lists
    for nprobe in (1, SK):
        want = _brute_shortlist(index, C, Q, S, nprobe, dtype)
        got = ops.pq_shortlist(index, Q, C, S, nprobe)
        assert got.dtype == torch.int64 and got.shape == (Q.shape[0], nprobe * S)
        assert torch.equal(got, want), (S, nprobe)
    # the long list fills every group; the short ones only the first
    got = ops.pq_shortlist(index, Q[:1], C, S, 1).view(-1)
    assert int((got >= 0).sum()) == S
    near_empty = ops.pq_shortlist(index, Q[-1:], C, S, 1)
    assert bool((near_empty == -1).all())


@pytest.mark.parametrize("S", [1, 32, 64, 256])
def test_shortlist_does_not_depend_on_the_blocking(lists, S):
    dtype, C, X, index, Q = lists
    want = ops.pq_shortlist(index, Q, C, S, 3)
    for block in (1, 3, Q.shape[0]):
        assert torch.equal(ops.pq_shortlist(index, Q, C, S, 3, block_queries=block), want), block


def test_shortlist_argument(lists):
    dtype, C, X, index, Q = lists
    for S in (0, 33, 48, 63, 288, 512, -1):
        with pytest.raises(ValueError, match=r"1 <= shortlist <= 32.*64, 96, 128, 160, 192, 224, 256"):
            ops.pq_shortlist(index, Q, C, S, 1)
    assert [ops.pq_shortlist_groups(S) for S in (1, 5, 32, 64, 96, 256)] == [(1, 1), (1, 5), (1, 32), (2, 32), (3, 32), (8, 32)]


# ---------------------------------------------------------------- integer coordinates: every operation exact
@pytest.fixture(scope="module")
def exact():
    g = torch.Generator().manual_seed(7)
    X = torch.randint(-8, 9, (640, 24), generator=g).to(torch.float32)
    km = mikmeans.KMeans(64, dtype="float32", device="cpu", seed=1)
    km.cluster_centers_ = X[:64].clone()
    ix = km.build_pq_index(X, 8, train_rows=640, pq_max_iter=2)
    assert int(ix.list_sizes.max()) <= 32                                            # the precondition
    Q = torch.randint(-8, 9, (48, 24), generator=torch.Generator().manual_seed(8)).to(torch.float32)
    d = ((Q.double()[:, None, :] - X.double()[None, :, :]) ** 2).sum(-1)             # [nq, n], exact
    order = torch.argsort(d, dim=1, stable=True)                                     # by (distance, row id)
    return km, ix, X, Q, d, order


@pytest.mark.parametrize("m", [1, 10, 32])
def test_integer_data_full_probe_is_the_exact_search(exact, m):
    km, ix, X, Q, d, order = exact
    rows, d2 = ix.search(Q, m, nprobe=64, squared=True, refine=X, shortlist=32)
    assert torch.equal(rows, order[:, :m])
    assert torch.equal(d2.double(), d.gather(1, order[:, :m]))


@pytest.mark.parametrize("nprobe,S,m", [(4, 10, 10), (4, 32, 10), (8, 5, 5), (8, 64, 32), (1, 32, 3), (16, 1, 1)])
def test_integer_data_refine_keeps_every_true_neighbour_the_codes_found(exact, nprobe, S, m):
    km, ix, X, Q, d, order = exact
    plain, _ = ix.search(Q, m, nprobe=nprobe)
    fine, _ = ix.search(Q, m, nprobe=nprobe, refine=X, shortlist=S)
    for q in range(Q.shape[0]):
        truth = set(order[q, :m].tolist())
        held = truth & set(plain[q].tolist())
        assert held <= set(fine[q].tolist()), (q, sorted(held - set(fine[q].tolist())))


# ---------------------------------------------------------------- the public interface
def test_search_without_refine_is_unchanged(exact):
    km, ix, X, Q, d, order = exact
    rows, d2 = ix.search(Q, 7, nprobe=5, squared=True)
    r0, d0 = ops.index_decode(ops.pq_search(ix._index, Q, km.cluster_centers_, 7, 5))
    assert torch.equal(rows, r0) and torch.equal(d2.view(torch.int32), d0.view(torch.int32))
    rows1, d1 = ix.search(Q, 7, nprobe=5, squared=True, refine=None, shortlist=None)
    assert torch.equal(rows1, rows) and torch.equal(d1.view(torch.int32), d2.view(torch.int32))


def test_refined_search_is_the_rerank_of_the_shortlist(exact):
    km, ix, X, Q, d, order = exact
    c = km.cluster_centers_
    cand = ops.pq_shortlist(ix._index, Q, c, 12, 6)
    r0, d0 = ops.index_decode(ops.rerank(Q, X, cand, 9))
    rows, d2 = ix.search(Q, 9, nprobe=6, squared=True, refine=X, shortlist=12)
    assert torch.equal(rows, r0) and torch.equal(d2.view(torch.int32), d0.view(torch.int32))
    rows1, d1 = ix.search(Q, 9, nprobe=6, refine=X, shortlist=12)
    assert torch.equal(rows1, rows) and torch.equal(d1.view(torch.int32), d0.sqrt().view(torch.int32))
    keys = ops.pq_refine(ix._index, Q, c, X, 9, 6, 12)
    for block in (1, 5):
        assert torch.equal(ops.pq_refine(ix._index, Q, c, X, 9, 6, 12, block_queries=block), keys)
    # the default shortlist is 32
    a = ix.search(Q, 9, nprobe=6, refine=X)
    b = ix.search(Q, 9, nprobe=6, refine=X, shortlist=32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_refined_search_errors(exact):
    km, ix, X, Q, d, order = exact
    for S in (0, 33, 100, 512):
        with pytest.raises(ValueError, match="shortlist"):
            ix.search(Q, 3, refine=X, shortlist=S)
    with pytest.raises(ValueError, match="only with refine"):
        ix.search(Q, 3, shortlist=32)
    for bad in (X[:-1], X[:, :-1], X.reshape(-1), X[None]):
        with pytest.raises(ValueError, match="refine takes the rows"):
            ix.search(Q, 3, refine=bad)
    for m in (0, 33):
        with pytest.raises(ValueError, match="1 <= m <= 32"):
            ix.search(Q, m, refine=X)
    with pytest.raises(ValueError, match="nprobe"):
        ix.search(Q, 3, nprobe=65, refine=X)
    cos = mikmeans.KMeans(64, dtype="float32", device="cpu", metric="cosine")
    cos.cluster_centers_ = torch.nn.functional.normalize(X[:64] + 0.5, dim=1)
    with pytest.raises(NotImplementedError, match="cosine"):
        mikmeans.PQIndex(cos, ix._index).search(Q, 3, refine=X)


def test_refined_search_pads_short_lists(exact):
    km, ix, X, Q, d, order = exact
    rows, dist = ix.search(Q, 32, nprobe=1, refine=X)
    sizes = ix.list_sizes[ops.topk(Q, km.cluster_centers_, 1)[0][:, 0].long()]
    assert bool((sizes < 32).any())
    assert torch.equal((rows >= 0).sum(1), sizes)
    assert bool(((rows == -1) == torch.isnan(dist)).all())
    for q in range(Q.shape[0]):
        k = int(sizes[q])
        assert bool((rows[q, :k] >= 0).all()) and bool((rows[q, k:] == -1).all())


def test_numpy_round_trip(exact):
    km, ix, X, Q, d, order = exact
    rows, dist = ix.search(Q, 6, nprobe=4, refine=X, shortlist=8)
    rn, dn = ix.search(Q.numpy(), 6, nprobe=4, refine=X.numpy(), shortlist=8)
    assert isinstance(rn, np.ndarray) and isinstance(dn, np.ndarray)
    assert np.array_equal(rn, rows.numpy()) and np.array_equal(dn.view(np.int32), dist.numpy().view(np.int32))
    # host rows of another float type are converted to the model's
    r64, d64 = ix.search(Q, 6, nprobe=4, refine=X.double().numpy(), shortlist=8)
    assert torch.equal(r64, rows) and torch.equal(d64.view(torch.int32), dist.view(torch.int32))


def test_command_line_round_trip(exact, tmp_path, capsys):
    from mikmeans.cli import main

    km, ix, X, Q, d, order = exact
    km.n_iter_, km.history_ = 1, []
    km.save(tmp_path / "ck")
    ix.save(tmp_path / "ix")
    np.save(tmp_path / "x.npy", X.numpy())
    np.save(tmp_path / "q.npy", Q.numpy())
    common = ["--model", str(tmp_path / "ck"), "--device", "cpu"]
    search = ["search", *common, "--queries", str(tmp_path / "q.npy"), "--nprobe", "4", "--top", "6"]
    pq = [*search, "--index", str(tmp_path / "ix")]
    assert main([*pq, "--refine", str(tmp_path / "x.npy"), "--shortlist", "8", "--output", str(tmp_path / "a.npz")]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["n_queries"] == Q.shape[0] and rec["top"] == 6
    got = np.load(tmp_path / "a.npz")
    rows, dist = ix.search(Q, 6, nprobe=4, refine=X, shortlist=8)
    assert np.array_equal(got["rows"], rows.numpy())
    assert np.array_equal(got["distances"].view(np.int32), dist.numpy().view(np.int32))
    assert main([*pq, "--refine", str(tmp_path / "x.npy"), "--output", str(tmp_path / "b.npz")]) == 0
    capsys.readouterr()
    r32, _ = ix.search(Q, 6, nprobe=4, refine=X)
    assert np.array_equal(np.load(tmp_path / "b.npz")["rows"], r32.numpy())
    with pytest.raises(SystemExit, match="--refine"):
        main([*pq, "--shortlist", "8"])
    with pytest.raises(SystemExit, match="shortlist"):
        main([*pq, "--refine", str(tmp_path / "x.npy"), "--shortlist", "48"])
    # a flat index takes neither flag
    flat = [*search, "--input", str(tmp_path / "x.npy")]
    with pytest.raises(SystemExit, match="PQ index"):
        main([*flat, "--refine", str(tmp_path / "x.npy")])
    with pytest.raises(SystemExit, match="PQ index"):
        main([*flat, "--shortlist", "8"])


def test_memory_plan_matches_the_tensors():
    from mikmeans.parallel import memplan

    n, F, K, M, nprobe, m = 10 ** 6, 128, 1024, 16, 16, 10
    for S in (5, 32, 256):
        for host in (False, True):
            B = ops.pq_refine_block_queries(M, nprobe, F, S, host_rows=host, esize=2)
            assert B == memplan.pq_refine_block_queries(M, nprobe, F, S, host_rows=host, esize=2) and B >= 1
            R = nprobe * S
            # a block's tables, scan keys, candidate ids, re-rank keys and their sort, and the staged rows
            per = nprobe * (M * 1024 + 8 * S) + 8 * R + 3 * 8 * R + (R * (F * 2 + 8) if host else 0)
            assert B * per <= ops.PQ_SCAN_BYTES
            plan = memplan.plan_pq_refine(n, F, K, M, torch.bfloat16, nq=10 ** 5, m=m, nprobe=nprobe, shortlist=S,
                                          host_rows=host)
            assert plan.mode == "pq-index-refine" and plan.fits
            blk = plan.transient["block"]
            # the tensors ops.pq_refine allocates for a block: [B * nprobe, G, s] scan keys, [B, R] ids and keys
            for name in ("shortlist_keys", "candidates", "rerank_keys", "sorted_keys", "sort_order"):
                assert blk[name] == memplan._r(B * R * 8), name
            assert blk["tables"] == memplan._r(B * nprobe * M * 1024)
            assert blk["block_keys"] == memplan._r(B * m * 8)
            assert ("staged_rows" in blk) == host
            if host:
                assert blk["staged_rows"] == memplan._r(min(B * R, n) * F * 2)
            assert plan.persistent["result_keys"] == memplan._r(10 ** 5 * m * 8)
            plain = memplan.plan_pq_search(n, F, K, M, torch.bfloat16, nq=10 ** 5, m=m, nprobe=nprobe)
            assert {k: plan.persistent[k] for k in plain.persistent} == plain.persistent
            plan.budget = plan.peak - 1
            assert not plan.fits
    assert ops.pq_refine_block_queries(M, nprobe, F, 256) < ops.pq_refine_block_queries(M, nprobe, F, 32)


def test_wiring():
    from mikmeans import _build

    assert "rerank.hip" in _build.HIP_SOURCES and (_build.CSRC / "rerank.hip").exists()
    assert (_build.CSRC / "rerankplan.h").exists()
    assert "-ffp-contract=off" in _build.source_flags("rerank.hip")
    for name in ("pq_shortlist", "pq_refine", "rerank", "pq_refine_block_queries"):
        assert name in ops.__all__ and getattr(ops, name) is not None
    src = (_build.CSRC / "binding.cpp").read_text()
    assert 'm.def("rerank"' in src
    assert "launch_rerank" in (_build.CSRC / "kernels.h").read_text()
    assert "for_type" in (_build.CSRC / "rerank.hip").read_text()


def test_rerank_kernels_spill_nothing_and_stay_under_128_vgprs(tmp_path):
    """Both dtypes, vector and element loads, of the built gfx950 object: no spills, no scratch, no
    static LDS and fewer than 128 VGPRs."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    ks = _kernels("rerank.hip", "rerank_kernel", tmp_path)                           # (T, VEC)
    assert set(ks) == {(t, v) for t in ("unsigned short", "float") for v in ("true", "false")}
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes, r.lds_bytes) for t, r in ks.items()
           if r.vgpr_spills or r.scratch_bytes or r.vgprs >= 128 or r.lds_bytes]
    assert not bad, bad


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_rerank_planning_under_asan_ubsan(tmp_path):
    """csrc/rerankplan.h: for edge and random (nq, R) the waves' runs, batches, steps and lane groups
    take every (query, candidate) exactly once; the run rule, the grid bound and the pieces of a row."""
    exe = tmp_path / "rerank_fuzz"
    src = os.path.join(ROOT, "tests", "native", "rerank_fuzz.cpp")
    inc = os.path.join(ROOT, "mikmeans", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", inc, src, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
