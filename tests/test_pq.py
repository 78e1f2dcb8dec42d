"""The product-quantised index on CPU tensors: the mirrors of mikmeans.ops.cpu against brute-force
torch definitions, the public interface, save / load, the command line, the memory plan and the
launch planning of csrc/pqplan.h under ASan + UBSan."""
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
K, F = 5, 16


def _data(dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = torch.randn(K, F, generator=g) * 12
    sizes = [0, 1, 70, 300, 129]
    lab = torch.repeat_interleave(torch.arange(K), torch.tensor(sizes))
    X = C[lab] + torch.randn(lab.numel(), F, generator=g)
    X = X[torch.randperm(X.shape[0], generator=g)]
    return C, X.to(dtype)


def _model(C, dtype):
    km = mikmeans.KMeans(K, dtype="bfloat16" if dtype == torch.bfloat16 else "float32", device="cpu")
    km.cluster_centers_ = C.clone()
    return km


def _books(C, X, M, dtype, seed=3):
    """Codebooks made of random listed rows' residual sub-vectors."""
    g = torch.Generator().manual_seed(seed)
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    R = (X.float() - C[lab]).to(dtype).float()
    pick = torch.randperm(X.shape[0], generator=g)[:256]
    return R[pick].view(256, M, F // M).permute(1, 0, 2).contiguous()


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def built(request):
    dtype = request.param
    C, X = _data(dtype)
    M = 8
    books = _books(C, X, M, dtype)
    index = ops.pq_build(X, C, M, codebooks=books)
    return dtype, C, X, M, books, index


def test_encode_is_the_nearest_codeword(built):
    dtype, C, X, M, books, index = built
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    R = (X.float() - C[lab]).to(dtype)
    codes = ops.pq_encode(R, books)
    assert codes.dtype == torch.uint8 and codes.shape == (X.shape[0], M)
    assert torch.equal(codes, cpu.pq_encode(R, books))
    dsub = F // M
    q = cpu.quantize_centers(books, dtype).double()
    for j in range(M):
        d = torch.cdist(R[:, j * dsub : (j + 1) * dsub].double(), q[j]) ** 2
        v, i = torch.sort(d, dim=1)
        # where float64 separates the two nearest codewords by more than float32 rounding, the code is the argmin
        clear = (v[:, 1] - v[:, 0]) > 1e-4 * (1 + v[:, 1])
        assert clear.sum() > 0.8 * clear.numel()
        assert torch.equal(codes[clear, j].long(), i[clear, 0])
        # and everywhere it is a codeword at (nearly) the least distance
        got = d.gather(1, codes[:, j : j + 1].long())[:, 0]
        assert bool((got <= v[:, 0] + 1e-4 * (1 + v[:, 0])).all())


def test_layout(built):
    dtype, C, X, M, books, index = built
    flat = ops.index_build(X, C)
    assert torch.equal(index.order, flat.order) and torch.equal(index.offsets, flat.offsets)
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    codes = ops.pq_encode((X.float() - C[lab]).to(dtype), books)
    for l in range(K):
        a, b = int(index.offsets[l]), int(index.offsets[l + 1])
        assert torch.equal(index.codes[a:b], codes[index.order[a:b]])
    assert index.codes.shape == (X.shape[0], M) and index.codes.is_contiguous()
    n, dsub = X.shape[0], F // M
    assert index.nbytes == n * M + 8 * n + 8 * (K + 1) + 4 * M * 256 * dsub
    # blocking changes nothing
    other = ops.pq_build(X, C, M, codebooks=books, block_rows=97)
    for a, b in zip(index.tensors().values(), other.tensors().values()):
        assert torch.equal(a, b)


def test_non_finite_rows_are_in_no_list(built):
    dtype, C, X, M, books, index = built
    X2 = X.clone()
    X2[5, 3] = float("nan")
    X2[77, 0] = float("inf")
    ix2 = ops.pq_build(X2, C, M, codebooks=books)
    assert int(ix2.offsets[-1]) == int(index.offsets[-1]) - 2
    assert not bool(((ix2.order == 5) | (ix2.order == 77)).any())
    nv = int(ix2.offsets[-1])
    assert bool((ix2.order[nv:] == -1).all()) and bool((ix2.codes[nv:] == 0).all())
    # every other row keeps its codes
    pos = {int(r): i for i, r in enumerate(index.order.tolist())}
    keep = torch.tensor([pos[int(r)] for r in ix2.order[:nv].tolist()])
    assert torch.equal(ix2.codes[:nv], index.codes[keep])


def _brute(index, C, Q, m, nprobe, dtype):
    """Search keys by the definitions, one pair and one row at a time in torch scalars' order of adds."""
    M, dsub = index.M, F // index.M
    probes = ops.topk(Q, C, nprobe)[0].long()
    nq = Q.shape[0]
    out = torch.full((nq, m), cpu.IVF_EMPTY_KEY, dtype=torch.int64)
    # the tables of all pairs at once: off the GPU transform is cdist, whose bits are the batch's own
    RQ = (Q.float()[:, None, :] - C[probes]).to(dtype).view(nq * nprobe, F)
    luts = torch.stack([ops.transform(RQ[:, s * dsub : (s + 1) * dsub], index.codebooks[s], squared=True)
                        for s in range(M)], dim=1)                       # [npairs, M, 256]
    assert torch.equal(luts, ops.pq_lut(RQ, index.codebooks)) and bool((luts >= 0).all())
    for q in range(nq):
        keys = []
        for j in range(nprobe):
            l = int(probes[q, j])
            lut = luts[q * nprobe + j]
            a, b = int(index.offsets[l]), int(index.offsets[l + 1])
            if a == b:
                continue
            c = index.codes[a:b].long()
            acc = lut[0][c[:, 0]]
            for s in range(1, M):
                acc = torch.add(acc, lut[s][c[:, s]])
            keys.append((acc.view(torch.int32).to(torch.int64) << 32) | index.order[a:b])
        if keys:
            k = torch.cat(keys).sort().values[:m]
            out[q, : k.numel()] = k
    return out


@pytest.mark.parametrize("m,nprobe", [(1, 1), (8, 2), (9, K), (32, 1)])
def test_search_keys_follow_the_sequential_add_rule(built, m, nprobe):
    dtype, C, X, M, books, index = built
    g = torch.Generator().manual_seed(5)
    Q = torch.cat([X[torch.randperm(X.shape[0], generator=g)[:21]].float() + 0.05, C[:2] + 0.05]).to(dtype)
    keys = ops.pq_search(index, Q, C, m, nprobe)
    assert keys.dtype == torch.int64 and keys.shape == (23, m)
    # (one call, one block: off the GPU the tables are cdist's, whose bits depend on the batch;
    # tests/test_gpu_pq.py has the blocking and single-query identities of the kernels)
    assert torch.equal(keys, _brute(index, C, Q, m, nprobe, dtype))
    assert torch.equal(keys, ops.pq_search(index, Q, C, m, nprobe))
    if nprobe == 1 and m == 32:
        assert bool((keys[21] == cpu.IVF_EMPTY_KEY).all())          # the empty list
        assert int((keys[22] != cpu.IVF_EMPTY_KEY).sum()) == 1      # the 1-row list
    rows, d2 = ops.index_decode(keys)
    assert bool(((rows >= 0) | torch.isnan(d2)).all())


def test_training_is_reproducible_and_lowers_the_error():
    C, X = _data(torch.float32, seed=1)
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    R = X.float() - C[lab]
    M = 8
    a = ops.pq_train(R, M, max_iter=4, seed=7)
    b = ops.pq_train(R, M, max_iter=4, seed=7)
    assert a.shape == (M, 256, F // M) and a.dtype == torch.float32 and torch.equal(a, b)

    def mse(books):
        codes = ops.pq_encode(R, books).long()
        rec = books[torch.arange(M)[None, :], codes].reshape(R.shape[0], F)
        return float(((rec.double() - R.double()) ** 2).sum(1).mean())

    first = R[:256].view(256, M, F // M).permute(1, 0, 2).contiguous()
    assert mse(a) < mse(first)
    with pytest.raises(ValueError, match="at least 256"):
        ops.pq_train(R[:255], M)


def test_api_save_load_and_reconstruct(built, tmp_path):
    dtype, C, X, M, books, index = built
    km = _model(C, dtype)
    ix = km.build_pq_index(X, M, codebooks=books)
    assert isinstance(ix, mikmeans.PQIndex) and ix.n_rows == X.shape[0] and ix.n_subvectors == M
    assert ix.n_indexed == int(index.offsets[-1]) and ix.nbytes == index.nbytes
    assert torch.equal(ix.list_sizes, index.offsets[1:] - index.offsets[:-1])
    assert torch.equal(ix.rows_of(3), index.order[int(index.offsets[3]) : int(index.offsets[4])])
    Q = X[:19]
    rows, d = ix.search(Q, 6, nprobe=3, squared=True)
    r0, d0 = ops.index_decode(ops.pq_search(index, Q, C, 6, 3))
    assert torch.equal(rows, r0) and torch.equal(d.view(torch.int32), d0.view(torch.int32))
    rn, dn = ix.search(Q.float().numpy(), 6, nprobe=3)
    assert isinstance(rn, np.ndarray) and isinstance(dn, np.ndarray)
    assert np.array_equal(rn, rows.numpy()) and np.array_equal(dn.view(np.int32), d.sqrt().numpy().view(np.int32))
    # reconstruct: the centre plus the codewords; NaN for an id in no list
    ids = torch.tensor([0, 7, X.shape[0] - 1])
    lab = ops.topk(X, C, 1)[0][:, 0].long()
    codes = ops.pq_encode((X.float() - C[lab]).to(dtype), books).long()
    want = C[lab[ids]] + books[torch.arange(M)[None, :], codes[ids]].reshape(3, F)
    assert torch.equal(ix.reconstruct(ids), want)
    assert bool(torch.isnan(ix.reconstruct(torch.tensor([X.shape[0] + 5]))).all())
    # save / load
    ix.save(tmp_path / "pq")
    assert mikmeans.PQIndex.saved_at(tmp_path / "pq") and not mikmeans.ClusterIndex.saved_at(tmp_path / "pq")
    assert json.loads((tmp_path / "pq" / "pq_index.json").read_text())["format"] == "mikmeans-pq-index-v1"
    back = km.load_pq_index(tmp_path / "pq")
    r2, d2 = back.search(Q, 6, nprobe=3, squared=True)
    assert torch.equal(r2, rows) and torch.equal(d2.view(torch.int32), d.view(torch.int32))
    with pytest.raises(ValueError, match="centres"):
        _model(C + 1, dtype).load_pq_index(tmp_path / "pq")
    # the functional form
    fx = mikmeans.build_pq_index(X, C, M, dtype="bfloat16" if dtype == torch.bfloat16 else "float32", codebooks=books)
    assert torch.equal(fx._index.codes, index.codes)


def test_api_trains_from_the_models_seed(built):
    dtype, C, X, M, books, index = built
    km = _model(C, dtype)
    a = km.build_pq_index(X, M, train_rows=300, pq_max_iter=2)
    b = km.build_pq_index(X, M, train_rows=300, pq_max_iter=2, block_rows=111)
    assert torch.equal(a.codebooks, b.codebooks) and torch.equal(a._index.codes, b._index.codes)
    assert a.codebooks.shape == (M, 256, F // M)


def test_errors(built):
    dtype, C, X, M, books, index = built
    km = _model(C, dtype)
    with pytest.raises(ValueError, match=r"\(8, 16, 32, 64\)"):
        km.build_pq_index(X, 12)
    with pytest.raises(ValueError, match=r"\(8, 16, 32, 64\)"):
        km.build_pq_index(X, 32)                      # 16 % 32 != 0
    with pytest.raises(ValueError, match="at least 256"):
        km.build_pq_index(X[:200], M)
    ix = km.build_pq_index(X, M, codebooks=books)
    for m in (0, 33):
        with pytest.raises(ValueError, match="1 <= m <= 32"):
            ix.search(X[:3], m)
    for nprobe in (0, K + 1):
        with pytest.raises(ValueError, match="nprobe"):
            ix.search(X[:3], 1, nprobe=nprobe)
    with pytest.raises(ValueError, match="features"):
        ops.pq_search(index, X[:3, :8], C, 1, 1)
    other = torch.float32 if dtype == torch.bfloat16 else torch.bfloat16
    with pytest.raises(ValueError, match="features"):
        ops.pq_search(index, X[:3].to(other), C, 1, 1)
    with pytest.raises(ValueError, match="codebooks must be"):
        ops.pq_build(X, C, M, codebooks=books[:, :100])


def test_multi_rank_jobs_are_refused(built):
    dtype, C, X, M, books, index = built

    class Grouped:
        rank, world, grouped = 0, 2, True

        def allreduce_(self, t):
            return t

    km = _model(C, dtype)
    km.comm = Grouped()
    with pytest.raises(NotImplementedError, match="multi-rank"):
        km.build_pq_index(X, M, codebooks=books)


def test_command_line_round_trip(tmp_path, capsys):
    from mikmeans.cli import main

    C, X = _data(torch.float32, seed=2)
    km = _model(C, torch.float32)
    km.n_iter_, km.history_ = 1, []
    km.save(tmp_path / "ck")
    np.save(tmp_path / "x.npy", X.numpy())
    np.save(tmp_path / "q.npy", X[:11].numpy())
    common = ["--model", str(tmp_path / "ck"), "--device", "cpu"]
    assert main(["index", *common, "--input", str(tmp_path / "x.npy"), "--output", str(tmp_path / "ix"), "--pq", "8",
                 "--train-rows", "300"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    n = X.shape[0]
    assert rec["n_rows"] == n and rec["n_subvectors"] == 8
    assert rec["nbytes"] == n * 8 + 8 * n + 8 * (K + 1) + 4 * 8 * 256 * 2
    search = ["search", *common, "--queries", str(tmp_path / "q.npy"), "--index", str(tmp_path / "ix"), "--nprobe", "2"]
    assert main([*search, "--top", "4", "--output", str(tmp_path / "a.npz")]) == 0
    got = np.load(tmp_path / "a.npz")
    ix = mikmeans.KMeans.load(tmp_path / "ck", device="cpu").load_pq_index(tmp_path / "ix")
    rows, d = ix.search(X[:11].numpy(), 4, nprobe=2)
    assert np.array_equal(got["rows"], rows) and np.array_equal(got["distances"].view(np.int32), d.view(np.int32))
    with pytest.raises(SystemExit, match="PQ index"):
        main([*search, "--top", "4", "--deep"])
    with pytest.raises(SystemExit, match="PQ index"):
        main([*search, "--radius", "1.0"])
    with pytest.raises(SystemExit, match="8, 16, 32, 64"):
        main(["index", *common, "--input", str(tmp_path / "x.npy"), "--output", str(tmp_path / "iy"), "--pq", "12"])


def test_memory_plan_matches_the_tensors(built):
    from mikmeans.parallel import memplan

    dtype, C, X, M, books, index = built
    n = X.shape[0]
    plan = memplan.plan_pq_index(n, F, K, M, dtype)
    assert plan.mode == "pq-index" and set(plan.persistent) == set(index.tensors())
    for name, t in index.tensors().items():
        assert plan.persistent[name] == memplan._r(t.untyped_storage().nbytes()), name
    assert set(plan.transient) == {"lists", "train", "encode"} and plan.fits
    plan.budget = plan.peak - 1
    assert not plan.fits
    sp = memplan.plan_pq_search(n, F, K, M, dtype, nq=1000, m=10, nprobe=3)
    B = ops.pq_block_queries(M, 10, 3, F)
    assert B == memplan.pq_block_queries(M, 10, 3, F) and B >= 1
    assert sp.transient["block"]["tables"] == memplan._r(min(1000, B) * 3 * M * 1024)
    assert sp.persistent["result_keys"] == memplan._r(1000 * 10 * 8)
    # a block's tables and keys stay under the byte budget
    pairs = B * 3
    assert pairs * (M * 1024 + 8 * 8 * 10) <= ops.PQ_SCAN_BYTES


def test_wiring():
    from mikmeans import _build

    assert "pq.hip" in _build.HIP_SOURCES and (_build.CSRC / "pq.hip").exists() and (_build.CSRC / "pqplan.h").exists()
    for name in ("pq_train", "pq_encode", "pq_lut", "pq_build", "pq_search", "PQRowIndex"):
        assert name in ops.__all__ and getattr(ops, name) is not None
    assert "build_pq_index" in mikmeans.__all__ and "PQIndex" in mikmeans.__all__
    assert hasattr(mikmeans.MiniBatchKMeans, "build_pq_index")
    src = (_build.CSRC / "binding.cpp").read_text()
    assert 'm.def("pq_scan"' in src and 'm.def("pq_scan_splits"' in src
    assert "launch_pq_scan" in (_build.CSRC / "kernels.h").read_text()
    assert ops.PQ_SUBVECTORS == (8, 16, 32, 64) and ops.PQ_KSUB == 256


def test_scan_kernels_spill_nothing_and_stay_under_128_vgprs(tmp_path):
    """Every instantiation (M sub-vectors, ML list length) of the built gfx950 object: no spills, no
    scratch and fewer than 128 VGPRs, so two workgroups' waves fit a SIMD; its LDS is all dynamic."""
    from mikmeans import _build
    from mikmeans.utils.isa import kernels as _kernels

    if shutil.which(_build._hipcc()) is None and not os.path.exists(_build._hipcc()):
        pytest.skip("hipcc not available")
    scan = _kernels("pq.hip", "pq_scan_kernel", tmp_path)                # (M, ML)
    assert set(scan) == {(str(M), str(ML)) for M in (8, 16, 32, 64) for ML in (8, 16, 32)}
    bad = [(t, r.vgprs, r.vgpr_spills, r.scratch_bytes, r.lds_bytes) for t, r in scan.items()
           if r.vgpr_spills or r.scratch_bytes or r.vgprs >= 128 or r.lds_bytes]
    assert not bad, bad


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_scan_planning_under_asan_ubsan(tmp_path):
    """csrc/pqplan.h: for random list lengths and every split count the waves' chunks cover every
    chunk and every row of a list exactly once; the split rule, the LDS bytes and the grid bound."""
    exe = tmp_path / "pq_fuzz"
    src = os.path.join(ROOT, "tests", "native", "pq_fuzz.cpp")
    inc = os.path.join(ROOT, "mikmeans", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", inc, src, "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]
