"""Rows, centres and queries with NaN or infinite coordinates through the distance kernels
(csrc/transform.hip, csrc/topk.hip, the scan of csrc/ivf.hip) and everything that folds their
output: cluster_report, cluster_exemplars, cluster_quantiles, build_index / search.

The oracle is independence from the poison.  A row's distances depend on that row and the centres
only, so with a few rows of ``X`` poisoned every other row must come out bit for bit as it does
from the clean ``X`` (the same tensor with the poisoned rows set to zero rows, which takes no
non-finite value anywhere), every poisoned row must come out NaN or inf -- never 0 -- and every
fold over ``X`` must equal the fold over the finite subset ``X[keep]`` with its row ids mapped
back.  (The folds' own filter on hand-made (idx, d2): test_gpu_quality.py, test_gpu_exemplars.py,
test_gpu_quantiles.py; the CPU mirrors under the same contract: test_topk.py, test_quality.py,
test_ivf.py.)"""
import functools

import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.ops import cpu as ref
from mikmeans.ops import pad_columns

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = [torch.float32, torch.bfloat16]
NAN, INF = float("nan"), float("inf")

# (n, D, K, m): a ragged single wave; D -> DPAD 32 with the M = 8 and the M = 32 list; DPAD 384 with
# the rows in registers; DPAD 1024, where bf16 m = 32 and f32 at both m fetch the row pieces again
# for every tile; a batch past the launcher's small-batch rule (several row blocks a wave); rows
# wider than the kernels (the torch mirror on the device)
TILES = [(70, 24, 7, 3), (513, 30, 37, 8), (513, 30, 37, 9), (300, 300, 20, 16), (200, 1024, 33, 8),
         (200, 1024, 33, 32), (131089, 64, 40, 8), (150, 1100, 4, 3)]
NARROW, RAGGED, WIDE = (513, 30, 37), (300, 300, 20), (200, 1024, 33)
KINDS = "abcde"


def _poison(X, row, kind):
    """One row made non-finite: a one NaN feature, b NaN in the last real column (before the pad
    columns at D = 30 / 300), c every feature +inf, d a single -inf, e one feature 1e20 (finite,
    but |x|^2 overflows to +inf)."""
    if kind == "a":
        X[row, 3] = NAN
    elif kind == "b":
        X[row, X.shape[1] - 1] = NAN
    elif kind == "c":
        X[row] = INF
    elif kind == "d":
        X[row, 5] = -INF
    else:
        X[row, 7] = 1e20


def _positions(n):
    """Row 0, the two sides of a 16-row block, one row in the middle -- off the first block of
    its wave where the wave holds several -- and the last row (lanes past n read it again)."""
    return [0, 15, 16, n // 2 + (21 if n >= 150 else 0), n - 1]


@functools.lru_cache(maxsize=None)
def _data(n, d, K, dtype, nq=40):
    """Rows around well-separated centres (C = 8 randn, rows C[lab] + 0.25 randn, every cluster
    populated) and queries near rows; never modified."""
    g = torch.Generator().manual_seed(n + 7 * K + d)
    C = 8.0 * torch.randn(K, d, generator=g)
    lab = (torch.arange(n) % K)[torch.randperm(n, generator=g)]
    X = (C[lab] + 0.25 * torch.randn(n, d, generator=g)).to(dtype)
    Q = (X[torch.randint(0, n, (nq,), generator=g)].float() + 0.25 * torch.randn(nq, d, generator=g)).to(dtype)
    return X.to(DEV), C.to(DEV), Q.to(DEV)


@functools.lru_cache(maxsize=None)
def _poisoned(n, d, K, dtype, turn=0):
    """(X with one row of each kind poisoned, the clean X, C, the poisoned rows, keep): the kinds
    go to the positions in an order that ``turn`` rotates."""
    X0, C, _ = _data(n, d, K, dtype)
    rows = _positions(n)
    assert len(set(rows)) == len(KINDS) and max(rows) == n - 1
    X, clean = X0.clone(), X0.clone()
    for j, row in enumerate(rows):
        _poison(X, row, KINDS[(j + turn) % len(KINDS)])
    bad = torch.tensor(rows, device=DEV)
    clean[bad] = 0
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    keep[bad] = False
    assert bool(torch.isfinite(clean.float()).all()) and bool(torch.isfinite(C).all())
    return X, clean, C, bad, keep


def _bits(t):
    """A tensor's bit patterns (so that NaN compares equal to itself and -0 differs from +0)."""
    t = torch.as_tensor(t)
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def _same(a, b):
    a, b = torch.as_tensor(a), torch.as_tensor(b)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a).cpu(), _bits(b).cpu())


# ------------------------------------------------------------------- transform, top-k
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("turn,shape", list(enumerate(TILES)))
def test_transform_poisoned_rows_are_nonfinite_and_alone(native, dtype, turn, shape):
    n, d, K, _ = shape
    X, clean, C, bad, keep = _poisoned(n, d, K, dtype, turn)
    for squared in (True, False):
        out = ops.transform(X, C, squared=squared)
        exp = ops.transform(clean, C, squared=squared)
        assert out.shape == (n, K) and bool(torch.isfinite(exp).all())
        finite = torch.isfinite(out[bad])
        assert not bool(finite.any()), (finite.any(dim=1).tolist(), out[bad][finite][:8].tolist())
        assert torch.equal(_bits(out[keep]), _bits(exp[keep])), int((_bits(out[keep]) != _bits(exp[keep])).sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("turn,shape", list(enumerate(TILES)))
def test_topk_poisoned_rows_are_nonfinite_and_alone(native, dtype, turn, shape):
    n, d, K, m = shape
    X, clean, C, bad, keep = _poisoned(n, d, K, dtype, turn)
    idx, d2 = ops.topk(X, C, m)
    ei, ed = ops.topk(clean, C, m)
    assert idx.shape == d2.shape == (n, m) and bool(torch.isfinite(ed).all())
    assert not bool(torch.isfinite(d2[bad, 0]).any()), d2[bad, 0].tolist()
    assert int(idx.min()) >= 0 and int(idx.max()) < K          # the poisoned rows too: no pad, no empty slot
    # (idx of a poisoned row is not pinned: the order of inf and NaN candidates is the kernel's own)
    assert torch.equal(idx[keep], ei[keep]), int((idx[keep] != ei[keep]).sum())
    assert torch.equal(_bits(d2[keep]), _bits(ed[keep])), int((_bits(d2[keep]) != _bits(ed[keep])).sum())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K", [NARROW, WIDE, (70, 24, 7)])
def test_nan_centre_is_never_near(native, dtype, n, d, K):
    """One NaN in centre k: column k of the transform is NaN, the other columns do not change, and
    the top-k lists are the stable sort of that matrix (NaN behind every number): centre k is the
    last of K and in no shorter list.  (At K = 37 and 33 the list of all K is the sorted transform;
    K = 7 puts the NaN centre into the kernel's own list.)"""
    X, C, _ = _data(n, d, K, dtype)
    T = ops.transform(X, C, squared=True)
    D0 = ops.transform(X, C)
    for k in (0, 5, K - 1):
        C2 = C.clone()
        C2[k, 2] = NAN
        others = torch.arange(K, device=DEV) != k
        for squared, exp in ((True, T), (False, D0)):
            got = ops.transform(X, C2, squared=squared)
            assert bool(got[:, k].isnan().all()), k
            assert torch.equal(_bits(got[:, others]), _bits(exp[:, others])), k
        Tk = T.clone()
        Tk[:, k] = NAN
        v, i = torch.sort(Tk, dim=1, stable=True)
        assert bool((i[:, K - 1] == k).all())
        for m in (K, 32, 8):       # every centre, then the kernel's M = 32 and M = 8 lists
            if m > K:
                continue
            idx, d2 = ops.topk(X, C2, m)
            c = min(m, K - 1)
            assert torch.equal(idx[:, :c].long(), i[:, :c]), (k, m)
            assert torch.equal(_bits(d2[:, :c]), _bits(v[:, :c])), (k, m)
            assert not bool((idx[:, :c] == k).any())
            if m == K:
                assert bool((idx[:, K - 1] == k).all()) and bool(d2[:, K - 1].isnan().all()), k


# ---------------------------------------------------------------------------- the folds
def _model(C, dtype):
    km = mikmeans.KMeans(C.shape[0], dtype="bfloat16" if dtype == torch.bfloat16 else "float32")
    km.cluster_centers_ = C
    return km


REPORT = ("counts", "cluster_inertia", "mean_distance", "rms_distance", "radius", "cluster_silhouette")


def _folds(km, X, Q, **kw):
    """Everything the four public calls return for X, as CPU tensors by name."""
    out = {}
    rep = km.cluster_report(X, **kw)
    for name in (*REPORT, "n_nonfinite", "table"):
        out[name] = getattr(rep, name)
    out["inertia"] = torch.tensor([rep.inertia, rep.silhouette, rep.davies_bouldin], dtype=torch.float64)
    out["q_values"], out["q_counts"] = km.cluster_quantiles(X, (0, 0.5, 1), **kw)
    out["near_rows"], out["near_d"] = km.cluster_exemplars(X, 4, **kw)
    out["far_rows"], out["far_d"] = km.cluster_exemplars(X, 4, farthest=True, **kw)
    ix = km.build_index(X, **kw)
    out["order"], out["order_full"], out["offsets"] = ix.order, ix._index.order, ix.offsets
    out["found_rows"], out["found_d2"] = ix.search(Q, 8, nprobe=4, squared=True)
    return {name: torch.as_tensor(t).cpu() for name, t in out.items()}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("turn,shape", [(1, NARROW), (3, RAGGED)])
def test_folds_equal_the_finite_subset(native, dtype, turn, shape):
    n, d, K = shape
    X, _, C, bad, keep = _poisoned(n, d, K, dtype, turn)
    _, _, Q = _data(n, d, K, dtype)
    km = _model(C, dtype)
    ids = keep.nonzero().flatten().cpu()
    nbad = int(bad.numel())

    def mapped(rows):
        return torch.where(rows < 0, rows, ids[rows.clamp_min(0)])

    got = _folds(km, X, Q)
    sub = _folds(km, X[keep], Q)
    # cluster_report: the poisoned rows are counted as left out and touch nothing else
    assert int(got["n_nonfinite"].sum()) == nbad and int(sub["n_nonfinite"].sum()) == 0
    assert int(got["counts"].sum()) == n - nbad and int(got["counts"].min()) > 0
    for name in (*REPORT, "inertia"):
        assert _same(got[name], sub[name]), name
    words = torch.arange(ops.QUALITY_WORDS) != 15           # (which cluster takes a poisoned row's count is open)
    assert torch.equal(got["table"][:, words], sub["table"][:, words])
    assert int(got["table"][:, 15].sum()) == nbad
    # cluster_quantiles: they are not counted
    assert _same(got["q_values"], sub["q_values"]) and torch.equal(got["q_counts"], sub["q_counts"])
    assert torch.equal(got["q_counts"], got["counts"]) and bool(torch.isfinite(got["q_values"]).all())
    # cluster_exemplars: they are in no list, nearest or farthest
    for side in ("near", "far"):
        assert torch.equal(got[side + "_rows"], mapped(sub[side + "_rows"])), side
        assert _same(got[side + "_d"], sub[side + "_d"]), side
        assert bool((got[side + "_rows"] >= 0).all()) and bool(torch.isfinite(got[side + "_d"]).all())
    # build_index / search: in no list, found by no query
    assert torch.equal(got["order"], ids[sub["order"]]) and torch.equal(got["offsets"], sub["offsets"])
    assert got["order_full"].shape == (n,) and torch.equal(got["order_full"][: n - nbad], got["order"])
    assert bool((got["order_full"][n - nbad:] == -1).all())
    assert torch.equal(got["found_rows"], mapped(sub["found_rows"])) and _same(got["found_d2"], sub["found_d2"])
    assert bool((got["found_rows"] >= 0).all())
    for name in ("near_rows", "far_rows", "order_full", "found_rows"):
        assert not bool(torch.isin(got[name], bad.cpu()).any()), name
    # any blocking of the rows, and host rows (NumPy in, NumPy out): the same answers
    again = _folds(km, X, Q, block_rows=77)
    host = _folds(km, X.float().cpu().numpy(), Q.float().cpu().numpy())
    for name, t in got.items():
        assert _same(again[name], t), ("block_rows", name)
        assert _same(host[name], t), ("numpy", name)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,d,K", [NARROW, RAGGED])
def test_poisoned_queries_do_not_disturb_the_others(native, dtype, n, d, K):
    """Queries with a NaN feature (a) or all +inf (c) mixed into a batch: every other query gets
    the keys of a search without them; the poisoned ones, whose results are unspecified, only
    rows that exist or the empty slot."""
    X, C, Q0 = _data(n, d, K, dtype)
    nq = Q0.shape[0]
    Q = Q0.clone()
    rows = _positions(nq)
    for j, row in enumerate(rows):
        _poison(Q, row, "ac"[j % 2])
    bad = torch.tensor(rows, device=DEV)
    keep = torch.ones(nq, dtype=torch.bool, device=DEV)
    keep[bad] = False
    ix = ops.index_build(X, C)
    assert ix.native and int(ix.offsets[-1]) == n
    for m, nprobe in ((8, 4), (32, K)):
        keys = ops.index_search(ix, Q, C, m, nprobe)
        exp = ops.index_search(ix, Q[keep], C, m, nprobe)
        assert keys.shape == (nq, m) and torch.equal(keys[keep], exp), (m, nprobe)
        assert torch.equal(exp, ops.index_search(ix, Q0, C, m, nprobe)[keep])
        found, _ = ops.index_decode(keys)
        assert bool(((found[bad] == -1) | ((found[bad] >= 0) & (found[bad] < n))).all()), (m, nprobe)
    km = _model(C, dtype)
    fr, fd = km.build_index(X).search(Q, 8, nprobe=4, squared=True)
    er, ed = ops.index_decode(ops.index_search(ix, Q[keep], C, 8, 4))
    assert torch.equal(fr[keep], er) and _same(fd[keep], ed)
    assert bool(((fr[bad] >= -1) & (fr[bad] < n)).all())


# --------------------------------------------------------------------------- the assign
# (what, dtype, D, K, switch): bf16 packed keys; the value-only argmin (bf16 D = 64, K >= 2048);
# the exact f32 MFMA; wide rows; the persistent kernel on 3 workgroups with the caller's norms
ASSIGNS = [("keys", torch.bfloat16, 128, 37, None), ("varg", torch.bfloat16, 64, 2048, ("assign_varg", 1)),
           ("f32", torch.float32, 128, 37, None), ("wide", torch.bfloat16, 384, 37, None),
           ("persist", torch.bfloat16, 128, 192, ("assign_persist", 3))]


@pytest.mark.parametrize("what,dtype,d,K,switch", ASSIGNS, ids=[a[0] for a in ASSIGNS])
def test_assign_nonfinite_rows_leave_neighbours_alone(native, kvariant, what, dtype, d, K, switch):
    """predict(unassign_nonfinite=True) with one row of every kind inside the first 192 rows -- one
    workgroup of every geometry (192 to 512 rows), shared with clean rows, and at least one
    workgroup without poison behind it: the poisoned rows get -1 (kind e too: its squared norm is
    inf in float32, so no centre is its nearest), every other row the float64 argmin.
    (A NaN norm must not reach the workgroup's seed offset and an infinite one must send
    the workgroup to per-point offsets: csrc/assign16.hip.)  Nothing is asserted about distances,
    inertia or score on such input."""
    n = 1000
    g = torch.Generator().manual_seed(d + K)
    C = 8.0 * torch.randn(K, d, generator=g)
    lab = (torch.arange(n) % K)[torch.randperm(n, generator=g)]
    X = (C[lab] + 0.25 * torch.randn(n, d, generator=g)).to(dtype)
    rows = [0, 15, 16, 100, 150]
    clean = torch.ones(n, dtype=torch.bool)
    clean[rows] = False
    # the condition on the input: every finite row's two nearest centres are further apart than
    # 2^-11 (|x - c|^2 + 3 |x|^2), 64 times the resolution of the packed keys
    Xd, Cq = X.double(), ref.quantize_centers(C, dtype).double()
    D2 = (Xd * Xd).sum(1)[:, None] + (Cq * Cq).sum(1)[None, :] - 2 * (Xd @ Cq.T)
    two = D2.topk(2, dim=1, largest=False)
    need = 2.0 ** -11 * (two.values[:, 0] + 3 * (Xd * Xd).sum(1))
    assert bool((two.values[:, 1] - two.values[:, 0] > need)[clean].all())
    exp = torch.where(clean, two.indices[:, 0], -1)
    for j, row in enumerate(rows):
        _poison(X, row, KINDS[j])
    X, C = X.to(DEV), C.to(DEV)
    if switch:
        kvariant(*switch)
    if what == "persist":
        # the binding itself as test_gpu_assign_persist.py calls it: without the centre-split
        # scratch ops.assign gives a batch this small (it would take the split grid), four row
        # groups on three workgroups; then predict's mask on its labels
        Xp = pad_columns(X)
        pk = ops.pack_centers(C, Xp.shape[1], dtype, DEV)
        got = torch.full((n,), 3, dtype=torch.int32, device=DEV)
        slots = torch.zeros(native.NSLOT * native.SLOT_STRIDE, dtype=torch.float64, device=DEV)
        native.assign(Xp, pk.pack, pk.cn, ops.row_sqnorm(Xp), got, torch.empty(n, device=DEV), slots, pk.Kpad, pk.dpad,
                      True, None, None, None, None, False, None, None)
        got = got.masked_fill(~torch.isfinite(X.float().square().sum(dim=1)), -1)
    else:
        got = _model(C, dtype).predict(X, unassign_nonfinite=True)
    got = got.cpu().long()
    assert bool((got[rows] == -1).all())
    assert torch.equal(got, exp), (got != exp).nonzero().flatten().tolist()[:10]
