"""An index that changes and lasts, on the CPU mirrors: ops.index_add / ops.index_remove against
the existing build (the oracle: the updated index equals, tensor for tensor, the index built over
the same rows at once), ClusterIndex.add / remove / save / load, the ``mikmeans index`` command and
the update's memory plan.  The checks take a device, so tests/test_gpu_index_update.py runs the
same ones on the kernels."""
import functools
import json

import numpy as np
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref
from mikmeans.parallel import memplan

DTYPES = [torch.float32, torch.bfloat16]
# (D, K, where the list cases start, the long list's (old, new) sizes): DPAD 32, the base shape,
# ragged wide rows, DPAD 1024 -- between them every case below, a few hundred to 3000 rows
SHAPES = [(30, 7, 0, (300, 120)), (128, 37, 0, (1500, 700)), (300, 20, 3, (500, 200)), (1024, 5, 6, (250, 100))]
# (old, new) rows of a list: empty on either side, a partial tile filled exactly, a partial tile
# overflowing, a whole-tile boundary, nothing new
ADD_PAIRS = [(0, 0), (0, 1), (0, 17), (1, 15), (15, 1), (15, 2), (16, 0), (16, 1), (17, 16), (33, 31)]
# (rows of a list, the positions that leave): 17 -> 16 by a tile's first slot, 16 -> 15 by a tile's
# last slot, 33 -> 1, 16 -> 0 (the list empties), nothing removed
REMOVE_CASES = [(17, [0]), (16, [15]), (33, [p for p in range(33) if p != 16]), (16, list(range(16))), (20, [])]


def add_sizes(K, off, long):
    pairs = [ADD_PAIRS[(k + off) % len(ADD_PAIRS)] for k in range(K - 1)] + [long]
    return torch.tensor([p[0] for p in pairs]), torch.tensor([p[1] for p in pairs])


def remove_plan(K, off, long):
    """``(sizes [K], per list the positions that leave)``: the cases in turn, then the long list
    (the first and last slots of its first tiles, its last row and every seventh row)."""
    cases = [REMOVE_CASES[(k + off) % len(REMOVE_CASES)] for k in range(K - 1)]
    n = long[0]
    cases.append((n, sorted({0, 15, 16, 31, n - 1, *range(3, n, 7)})))
    return torch.tensor([c[0] for c in cases]), [c[1] for c in cases]


@functools.lru_cache(maxsize=None)
def centres(d, K):
    g = torch.Generator().manual_seed(7 * K + d)
    return 8.0 * torch.randn(K, d, generator=g)


def rows_of(C, sizes, dtype, seed):
    """Rows around the (well separated) centres with the prescribed list sizes, shuffled: ``(X, labels)``."""
    g = torch.Generator().manual_seed(seed)
    n = int(sizes.sum())
    lab = torch.repeat_interleave(torch.arange(C.shape[0]), sizes)[torch.randperm(n, generator=g)]
    return (C[lab] + 0.25 * torch.randn(n, C.shape[1], generator=g)).to(dtype), lab


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def assert_same_tensors(a, b):
    for name, t in a.tensors().items():
        assert torch.equal(t.view(torch.uint8), b.tensors()[name].view(torch.uint8)), name


def assert_index_equal(got, exp, ids=None):
    """``got`` equals ``exp`` (the oracle's build): offsets, the used part of the pack and of cn
    bitwise, the rest of the allocation untouched fill, and ``order`` -- as is, or ``exp``'s mapped
    through ``ids`` (the old id of each of the oracle's rows)."""
    K = exp.K
    assert (got.K, got.D, got.dtype, got.native, got.cols) == (exp.K, exp.D, exp.dtype, exp.native, exp.cols)
    assert torch.equal(got.offsets, exp.offsets) and torch.equal(got.tile_offsets, exp.tile_offsets)
    nv, rows = int(exp.offsets[K]), 16 * int(exp.tile_offsets[K])
    assert got.pack.numel() == ops.index_tiles(got.n, K) * 16 * got.cols and got.cn.numel() == ops.index_tiles(got.n, K) * 16
    assert torch.equal(bits(got.pack[: rows * got.cols]), bits(exp.pack[: rows * exp.cols]))
    assert torch.equal(bits(got.cn[:rows]), bits(exp.cn[:rows]))
    assert not bool(bits(got.pack[rows * got.cols :]).any())
    assert torch.equal(bits(got.cn[rows:]), bits(torch.full_like(got.cn[rows:], ref.PAD_SCORE)))
    want = exp.order[:nv] if ids is None else ids.to(exp.order.device)[exp.order[:nv]]
    assert got.order.numel() == got.n and torch.equal(got.order[:nv], want) and bool((got.order[nv:] == -1).all())


def list_sizes(ix):
    return (ix.offsets[1:] - ix.offsets[:-1]).cpu()


# ------------------------------------------------------------------------------ the checks
def check_add(dev, dtype, d, K, off, long):
    C = centres(d, K).to(dev)
    s0, s1 = add_sizes(K, off, long)
    X0, X1 = rows_of(C.cpu(), s0, dtype, 1)[0].to(dev), rows_of(C.cpu(), s1, dtype, 2)[0].to(dev)
    old = ops.index_build(X0, C)
    assert torch.equal(list_sizes(old), s0)
    keep = {k: t.clone() for k, t in old.tensors().items()}
    got = ops.index_add(old, X1, C)
    exp = ops.index_build(torch.cat([X0, X1]), C)
    assert torch.equal(list_sizes(exp), s0 + s1) and got.n == exp.n == int(s0.sum() + s1.sum())
    assert_index_equal(got, exp)
    for k, t in old.tensors().items():                                  # a new index: the old one is whole
        assert torch.equal(t.view(torch.uint8), keep[k].view(torch.uint8)), k
    for other in (ops.index_add(old, X1, C, block_rows=777), ops.index_add(old, X1, C)):   # any blocking, any run
        assert_same_tensors(got, other)
    return got


def check_add_batches(dev, dtype):
    """One row; rows that all go to one list; rows with NaN and inf (an id each, no list)."""
    d, K = 30, 7
    C = centres(d, K).to(dev)
    s0 = torch.tensor([0, 1, 15, 16, 17, 33, 100])
    X0 = rows_of(C.cpu(), s0, dtype, 3)[0].to(dev)
    old = ops.index_build(X0, C)
    one = rows_of(C.cpu(), torch.tensor([0, 0, 1, 0, 0, 0, 0]), dtype, 4)[0].to(dev)
    same = rows_of(C.cpu(), torch.tensor([0, 0, 0, 40, 0, 0, 0]), dtype, 5)[0].to(dev)
    bad = rows_of(C.cpu(), torch.tensor([2, 2, 2, 2, 2, 2, 2]), dtype, 6)[0].to(dev)
    bad[1, 3], bad[6, 0], bad[13, 29] = float("nan"), float("inf"), float("-inf")
    for X1, listed in ((one, 1), (same, 40), (bad, 11)):
        got = ops.index_add(old, X1, C)
        assert_index_equal(got, ops.index_build(torch.cat([X0, X1]), C))
        assert got.n == old.n + X1.shape[0] and int(got.offsets[-1]) == int(old.offsets[-1]) + listed
    none = ops.index_add(old, X0[:0], C)                                 # nothing new: the same lists
    assert_index_equal(none, old)


def remove_case(dev, dtype, d, K, off, long):
    C = centres(d, K).to(dev)
    sizes, leave = remove_plan(K, off, long)
    X, lab = rows_of(C.cpu(), sizes, dtype, 7)
    ids = torch.cat([(lab == k).nonzero().flatten()[torch.tensor(p, dtype=torch.int64)] for k, p in enumerate(leave)])
    return C, X.to(dev), sizes, ids


def check_remove(dev, dtype, d, K, off, long):
    C, X, sizes, ids = remove_case(dev, dtype, d, K, off, long)
    n = X.shape[0]
    built = ops.index_build(X, C)
    assert torch.equal(list_sizes(built), sizes)
    mask = torch.ones(n, dtype=torch.bool)
    mask[ids] = False
    keep = mask.nonzero().flatten()
    g = torch.Generator().manual_seed(11)
    ids = ids[torch.randperm(ids.numel(), generator=g)].to(dev)          # any order
    got, removed = ops.index_remove(built, ids)
    assert removed.dtype == torch.int64 and removed.dim() == 0 and removed.device == built.order.device
    assert int(removed) == ids.numel() and got.n == n
    exp = ops.index_build(X[keep.to(dev)], C)
    assert_index_equal(got, exp, keep)
    assert_same_tensors(got, ops.index_remove(built, ids)[0])            # any run
    return got, keep


def check_remove_ignores(dev, dtype):
    """Unsorted ids with duplicates, values out of range and a row in no list; the same ids again."""
    d, K = 30, 7
    C = centres(d, K).to(dev)
    X = rows_of(C.cpu(), torch.tensor([0, 1, 15, 16, 17, 33, 100]), dtype, 8)[0]
    X[40, 2] = float("nan")                                              # row 40 is in no list
    X = X.to(dev)
    built = ops.index_build(X, C)
    n = X.shape[0]
    ids = torch.tensor([77, 3, 40, 77, n, -1, 1 << 40, 120, 3, -(1 << 35), n + 5, 0], device=dev)
    got, removed = ops.index_remove(built, ids)
    assert int(removed) == 4                                             # 77, 3, 120, 0
    keep = torch.tensor([i for i in range(n) if i not in (77, 3, 120, 0)])
    assert_index_equal(got, ops.index_build(X[keep.to(dev)], C), keep)
    again, removed2 = ops.index_remove(got, ids)
    assert int(removed2) == 0
    assert_same_tensors(again, got)
    every, removed3 = ops.index_remove(got, torch.arange(n, device=dev))  # every row of the index
    assert int(removed3) == n - 5 and every.n == n
    assert_index_equal(every, ops.index_build(X[:0], C), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.index_remove(built, torch.tensor([1.0, 2.0], device=dev))


def check_sequence(dev, dtype):
    """add, remove, add: ids keep growing, removed ids are never reused, and the result is the
    rebuild on the rows that stay."""
    d, K = 128, 37
    C = centres(d, K).to(dev)
    s0, s1 = add_sizes(K, 0, (300, 100))
    Xa, Xb = rows_of(C.cpu(), s0, dtype, 12)[0].to(dev), rows_of(C.cpu(), s1, dtype, 13)[0].to(dev)
    Xc = rows_of(C.cpu(), s1.flip(0), dtype, 14)[0].to(dev)
    na, nb, nc = Xa.shape[0], Xb.shape[0], Xc.shape[0]
    ix = ops.index_add(ops.index_build(Xa, C), Xb, C)
    gone = torch.cat([torch.arange(0, na, 3), torch.arange(na, na + nb, 2)])
    ix, removed = ops.index_remove(ix, gone.to(dev))
    assert int(removed) == gone.numel()
    ix = ops.index_add(ix, Xc, C)
    assert ix.n == na + nb + nc
    mask = torch.ones(ix.n, dtype=torch.bool)
    mask[gone] = False
    keep = mask.nonzero().flatten()
    assert_index_equal(ix, ops.index_build(torch.cat([Xa, Xb, Xc])[keep.to(dev)], C), keep)


def model_for(C, dtype, metric="euclidean"):
    km = mikmeans.KMeans(C.shape[0], dtype="bfloat16" if dtype == torch.bfloat16 else "float32", metric=metric)
    km.cluster_centers_ = C
    return km


def mapped(rows, keep):
    return torch.where(rows < 0, rows, keep.to(rows.device)[rows.clamp_min(0)])


def assert_searches_equal(got, exp, Q, K, keep=None):
    """search (m = 8, 32; nprobe = 1, 4, K) and range_search (sorted and not) of ``got`` are bitwise
    those of ``exp``, a freshly built ClusterIndex, its row ids mapped through ``keep``."""
    same = (lambda r: r) if keep is None else (lambda r: mapped(r, keep))
    for m in (8, 32):
        for nprobe in (1, 4, K):
            (r, dd), (er, ed) = got.search(Q, m, nprobe=nprobe, squared=True), exp.search(Q, m, nprobe=nprobe, squared=True)
            assert torch.equal(r, same(er)) and torch.equal(dd.view(torch.int32), ed.view(torch.int32)), (m, nprobe)
    radius = float(exp.search(Q, 8, nprobe=K)[1][:, -1].nan_to_num(0).median())
    for sort in (True, False):
        (l, r, dd), (el, er, ed) = (ix.range_search(Q, radius, nprobe=4, sort=sort) for ix in (got, exp))
        assert int(el[-1]) > 0 and torch.equal(l, el) and torch.equal(r, same(er))
        assert torch.equal(dd.view(torch.int32), ed.view(torch.int32))


def check_end_to_end(dev, dtype):
    """ClusterIndex.add / remove: ids, counts, host and device input, and the searches."""
    d, K, off, long = SHAPES[1]
    C = centres(d, K).to(dev)
    km = model_for(C, dtype)
    s0, s1 = add_sizes(K, off, long)
    X0, X1 = rows_of(C.cpu(), s0, dtype, 1)[0].to(dev), rows_of(C.cpu(), s1, dtype, 2)[0].to(dev)
    n0, n1 = X0.shape[0], X1.shape[0]
    g = torch.Generator().manual_seed(5)
    Xall = torch.cat([X0, X1])
    Q = (Xall[torch.randint(0, n0 + n1, (200,), generator=g).to(dev)].float()
         + 0.25 * torch.randn(200, d, generator=g).to(dev)).to(dtype)
    ix = km.build_index(X0)
    assert ix.add(X1) == n0 and ix.n_rows == n0 + n1 == ix.n_indexed
    assert_searches_equal(ix, km.build_index(Xall), Q, K)
    host = km.build_index(X0)                                            # host rows in small blocks: the same index
    assert host.add(X1.float().cpu().numpy(), block_rows=777) == n0
    assert_same_tensors(ix._index, host._index)
    gone = torch.arange(1, n0 + n1, 3)
    assert ix.remove(gone.numpy()[::-1].copy()) == gone.numel() and ix.remove(gone.to(dev)) == 0
    assert ix.n_rows == n0 + n1 and ix.n_indexed == n0 + n1 - gone.numel()
    mask = torch.ones(n0 + n1, dtype=torch.bool)
    mask[gone] = False
    keep = mask.nonzero().flatten()
    assert_searches_equal(ix, km.build_index(Xall[keep.to(dev)]), Q, K, keep)
    assert ix.add(X1[:5]) == n0 + n1 and ix.n_rows == n0 + n1 + 5        # removed ids are never handed out again
    with pytest.raises(ValueError):
        ix.add(X1[:, :-1])
    with pytest.raises(ValueError):
        ix.remove(torch.tensor([0.5]))
    assert ix.n_rows == n0 + n1 + 5
    return km, ix, Q


def check_save_load(dev, dtype, tmp_path, other_dev):
    km, ix, Q = check_end_to_end(dev, dtype)
    K = km.cluster_centers_.shape[0]
    ix.save(tmp_path / "ix")
    meta = json.loads((tmp_path / "ix" / "index.json").read_text())
    assert meta["n"] == ix.n_rows and meta["K"] == K and meta["native"] == (dev != "cpu") and meta["row_start"] == 0
    assert {"format", "n", "K", "D", "dtype", "native", "cols", "row_start"} <= set(meta)
    for back in (km.load_index(tmp_path / "ix"), mikmeans.ClusterIndex.load(tmp_path / "ix", km)):
        assert back.n_rows == ix.n_rows and back.n_indexed == ix.n_indexed
        assert_same_tensors(back._index, ix._index)
        assert_searches_equal(back, ix, Q, K)
    off = km.cluster_centers_.clone()
    off.view(torch.int32)[3, 5] ^= 1                                     # one bit of one centre
    with pytest.raises(ValueError):
        mikmeans.ClusterIndex.load(tmp_path / "ix", model_for(off, dtype))
    with pytest.raises(ValueError):                                      # the model's dtype differs
        mikmeans.ClusterIndex.load(tmp_path / "ix", model_for(km.cluster_centers_, DTYPES[1 - DTYPES.index(dtype)]))
    with pytest.raises(ValueError):                                      # the feature count differs
        mikmeans.ClusterIndex.load(tmp_path / "ix", model_for(km.cluster_centers_[:, :-8].contiguous(), dtype))
    if other_dev is not None:                                            # across layouts
        with pytest.raises(ValueError):
            mikmeans.ClusterIndex.load(tmp_path / "ix", model_for(km.cluster_centers_.to(other_dev), dtype))


# ------------------------------------------------------------------------------ CPU mirrors
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,K,off,long", SHAPES)
def test_add_equals_the_rebuild(dtype, d, K, off, long):
    got = check_add("cpu", dtype, d, K, off, long)
    assert not got.native


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_one_row_one_list_and_nonfinite_rows(dtype):
    check_add_batches("cpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,K,off,long", SHAPES)
def test_remove_equals_the_rebuild_on_the_survivors(dtype, d, K, off, long):
    check_remove("cpu", dtype, d, K, off, long)


@pytest.mark.parametrize("dtype", DTYPES)
def test_remove_ignores_what_is_not_there(dtype):
    check_remove_ignores("cpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_add_remove_add(dtype):
    check_sequence("cpu", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_cluster_index_updates_save_and_load(dtype, tmp_path):
    check_save_load("cpu", dtype, tmp_path, None)


def test_cosine_models_add_unit_rows():
    d, K = 30, 7
    C = torch.nn.functional.normalize(centres(d, K), dim=1)
    km = model_for(C, torch.float32, metric="cosine")
    s0, s1 = add_sizes(K, 0, (120, 60))
    g = torch.Generator().manual_seed(21)
    X0 = (C[torch.repeat_interleave(torch.arange(K), s0)] + 0.02 * torch.randn(int(s0.sum()), d, generator=g)) * 3.0
    X1 = (C[torch.repeat_interleave(torch.arange(K), s1)] + 0.02 * torch.randn(int(s1.sum()), d, generator=g)) * 0.5
    ix = km.build_index(X0)
    assert ix.add(X1) == X0.shape[0]
    exp = km.build_index(torch.cat([X0, X1]))
    assert torch.equal(exp.list_sizes, s0 + s1)
    assert_index_equal(ix._index, exp._index)
    norms = ix._index.pack.view(-1, d)[: 16 * int(ix._index.tile_offsets[-1])].norm(dim=1)
    assert bool(((norms - 1).abs() < 1e-5)[ix._index.cn[: norms.numel()] < 1e29].all())   # unit rows


def test_multi_rank_jobs_refuse(monkeypatch, tmp_path):
    C = centres(30, 7)
    km = model_for(C, torch.float32)
    ix = km.build_index(rows_of(C, torch.tensor([5] * 7), torch.float32, 1)[0])

    class Grouped:
        grouped = True

        def allreduce_(self, t):
            return t

    ix._comm = Grouped()
    for name, call in (("add", lambda: ix.add(C)), ("remove", lambda: ix.remove([1])), ("save", lambda: ix.save(tmp_path / "x"))):
        with pytest.raises(NotImplementedError, match=name):
            call()
    km.comm = Grouped()
    with pytest.raises(NotImplementedError, match="load"):
        mikmeans.ClusterIndex.load(tmp_path / "x", km)


# ------------------------------------------------------------------------------ command line
def test_index_command_and_search_from_a_saved_index(tmp_path, capsys):
    from mikmeans.cli import main

    d, K = 30, 7
    C = centres(d, K)
    s0, s1 = add_sizes(K, 0, (200, 80))
    X0, X1 = rows_of(C, s0, torch.float32, 1)[0], rows_of(C, s1, torch.float32, 2)[0]
    km = model_for(C, torch.float32)
    km.n_iter_, km.history_ = 1, []
    km.save(tmp_path / "ck")
    np.save(tmp_path / "x0.npy", X0.numpy())
    np.save(tmp_path / "x1.npy", X1.numpy())
    np.save(tmp_path / "q.npy", X1[:40].numpy())
    common = ["--model", str(tmp_path / "ck"), "--device", "cpu"]
    assert main(["index", *common, "--input", str(tmp_path / "x0.npy"), "--output", str(tmp_path / "ix")]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["n_rows"] == rec["n_indexed"] == X0.shape[0] and rec["added_first_id"] is None and rec["removed"] is None
    assert rec["nbytes"] == km.build_index(X0).nbytes
    search = ["search", *common, "--queries", str(tmp_path / "q.npy"), "--top", "5", "--nprobe", "3"]
    assert main([*search, "--input", str(tmp_path / "x0.npy"), "--output", str(tmp_path / "a.npz")]) == 0
    assert main([*search, "--index", str(tmp_path / "ix"), "--output", str(tmp_path / "b.npz")]) == 0
    assert (tmp_path / "a.npz").read_bytes() == (tmp_path / "b.npz").read_bytes()
    radius = ["search", *common, "--queries", str(tmp_path / "q.npy"), "--radius", "2.0", "--nprobe", "3"]
    assert main([*radius, "--input", str(tmp_path / "x0.npy"), "--output", str(tmp_path / "c.npz")]) == 0
    assert main([*radius, "--index", str(tmp_path / "ix"), "--output", str(tmp_path / "d.npz")]) == 0
    assert (tmp_path / "c.npz").read_bytes() == (tmp_path / "d.npz").read_bytes()
    gone = np.arange(0, X0.shape[0], 4)
    np.save(tmp_path / "gone.npy", gone)
    capsys.readouterr()
    assert main(["index", *common, "--output", str(tmp_path / "ix"), "--remove", str(tmp_path / "gone.npy"),
                 "--add", str(tmp_path / "x1.npy")]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    n = X0.shape[0] + X1.shape[0]
    assert rec["n_rows"] == n and rec["n_indexed"] == n - gone.size and rec["added_first_id"] == X0.shape[0]
    assert rec["removed"] == gone.size
    mask = torch.ones(n, dtype=torch.bool)
    mask[torch.from_numpy(gone)] = False
    keep = mask.nonzero().flatten()
    assert_index_equal(km.load_index(tmp_path / "ix")._index, ops.index_build(torch.cat([X0, X1])[keep], C), keep)
    for bad in (["--input", str(tmp_path / "x0.npy"), "--index", str(tmp_path / "ix")], []):
        with pytest.raises(SystemExit):
            main([*search, *bad])
    with pytest.raises(SystemExit):
        main(["index", *common, "--output", str(tmp_path / "nothing")])


# ------------------------------------------------------------------------------ memory plan
def test_plan_index_update_is_pinned():
    r = memplan._r
    p = memplan.plan_index_update(3000, 3300, 128, 37, "bfloat16")
    rows0, rows1 = (3000 + 15 * 37) // 16 * 16, (3300 + 15 * 37) // 16 * 16
    assert p.persistent == {"old_row_pack": r(rows0 * 128 * 2), "old_cn": r(rows0 * 4), "old_order": r(3000 * 8),
                            "old_offsets": r(38 * 8), "old_tile_offsets": r(38 * 8), "row_pack": r(rows1 * 128 * 2),
                            "cn": r(rows1 * 4), "order": r(3300 * 8), "offsets": r(38 * 8), "tile_offsets": r(38 * 8)}
    assert p.transient == {"update": {"labels": r(3300 * 4), "row_pos": r(3300 * 8), "old_labels": r(3000 * 4),
                                      "old_row_pos": r(3000 * 8), "top1_idx": r(300 * 4), "top1_d2": r(300 * 4),
                                      "top1_xn": r(300 * 4), "top1_labels": r(300 * 4),
                                      "partition_cells": r(37 * 4 * 8)}}
    assert p.peak == sum(p.persistent.values()) + sum(p.transient["update"].values()) and p.mode == "index-update"
    # float32, D = 30 -> 32 columns, a remove (no new rows), rows in blocks
    q = memplan.plan_index_update(200000, 200000, 30, 1024, "float32", block_rows=777)
    rows = (200000 + 15 * 1024) // 16 * 16
    one = {"row_pack": r(rows * 32 * 4), "cn": r(rows * 4), "order": r(200000 * 8), "offsets": r(1025 * 8),
           "tile_offsets": r(1025 * 8)}
    assert q.persistent == {**{"old_" + k: v for k, v in one.items()}, **one}
    assert q.transient == {"update": {"labels": r(200000 * 4), "row_pos": r(200000 * 8), "old_labels": r(200000 * 4),
                                      "old_row_pos": r(200000 * 8), "top1_idx": 0, "top1_d2": 0, "top1_xn": 0,
                                      "top1_labels": 0, "partition_cells": r(1024 * 196 * 8)}}
    # what the plan says an index keeps is what plan_index says
    assert {k: v for k, v in q.persistent.items() if not k.startswith("old_")} == memplan.plan_index(200000, 30, 1024, "float32").persistent
