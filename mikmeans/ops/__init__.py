"""Op layer: natural-layout entry points over the gfx950 kernels.

GPU tensors run the hand-written HIP kernels of ``mikmeans._C`` (fail loudly if
the extension is missing); CPU tensors run :mod:`mikmeans.ops.cpu`, the plain
PyTorch reference of the same op (the test oracle and the demo-parity path,
BASELINE config 1).  There is no third backend.

* :func:`row_sqnorm`   K1  |x_i|^2
* :func:`assign`       K2  nearest centroid + squared distance (MFMA GEMM + argmin)
* :func:`cluster_sums` K3  per-cluster sums / counts (LDS scatter-add + f64 slab reduce)
* :class:`CentroidPack` K4 fragment-packed centroids for the assign kernel
"""
from __future__ import annotations

import torch

from . import cpu
from .native import available, dpad_for, dtype_code, require, vec_elems

__all__ = [
    "available",
    "require",
    "dpad_for",
    "vec_elems",
    "pad_columns",
    "pack_centers",
    "row_sqnorm",
    "assign",
    "cluster_sums",
    "CentroidPack",
    "quality_accumulate",
    "quality_decode",
    "cluster_quality",
    "exemplar_accumulate",
    "exemplar_decode",
    "cluster_exemplars",
    "quantile_state",
    "quantile_hist",
    "quantile_select",
    "cluster_quantiles",
]


def pad_columns(X: torch.Tensor, dtype: torch.dtype | None = None) -> torch.Tensor:
    """Return ``X`` in ``dtype`` with columns zero-padded to a 16-byte multiple.

    Zero columns change neither distances nor cluster sums; the GPU kernels need
    16-byte rows.  No copy when ``X`` already qualifies.
    """
    dtype = dtype or X.dtype
    v = vec_elems(dtype)
    n, d = X.shape
    dp = (d + v - 1) // v * v
    ok = X.dtype == dtype and d == dp and X.stride(1) == 1 and (n <= 1 or X.stride(0) % v == 0)
    if ok and X.data_ptr() % 16 == 0:
        return X
    out = torch.zeros((n, dp), dtype=dtype, device=X.device)
    out[:, :d] = X.to(dtype)
    return out


def row_sqnorm(X: torch.Tensor) -> torch.Tensor:
    if not X.is_cuda:
        return cpu.row_sqnorm(X)
    C = require()
    Xp = pad_columns(X)
    out = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
    C.row_sqnorm(Xp, out)
    return out


SPLIT_MAX_ROWS = 1 << 18   # assign16 splits the centre range only below ~1024 point blocks


class CentroidPack:
    """Centroids in the assign kernel's fragment-packed layout (see csrc/kernels.h).

    ``pack`` holds ``-2*c`` (bf16 or f32, as the points) and ``cn`` holds
    ``|c_q|^2`` of the quantised centroids, padded with a huge score for the
    rows between K and Kpad.
    """

    def __init__(self, K: int, D: int, dtype: torch.dtype, device):
        C = require()
        self._C = C
        self.K, self.D, self.dtype = K, D, dtype
        self.dpad = dpad_for(D, dtype)
        if self.dpad == 0:
            raise NotImplementedError(f"mikmeans: GPU assign supports D <= 1024 (got {D})")
        self.dt = dtype_code(dtype)
        self.Kpad = C.assign_kpad(self.dt, self.dpad, K)
        self._keys = None
        self.pack = torch.zeros(self.Kpad * self.dpad, dtype=dtype, device=device)
        self.cn = torch.zeros(C.assign_cn_len(self.Kpad), dtype=torch.float32, device=device)

    def load(self, centers: torch.Tensor) -> "CentroidPack":
        c = centers.to(device=self.pack.device, dtype=torch.float32).contiguous()
        assert c.shape == (self.K, self.D), (c.shape, self.K, self.D)
        self.finalize(0, None, c)
        return self

    def finalize(self, mode: int, packed, Cold, Cnew=None, frozen=None, mb_counts=None, shift=None,
                 counts=None, qshift=None):
        """K4: new centres from the all-reduced message (mode 1 Lloyd, 2 mini-batch) or
        pack-only (mode 0); always re-packs ``-2c`` / ``|c|^2`` for the next assign.
        ``qshift``: the squared move of the quantised centres the assign ranks."""
        self._C.finalize(mode, packed, Cold, Cnew, frozen, mb_counts, self.pack, self.cn, shift, counts,
                         self.dpad, self.Kpad, qshift)

    def assign(self, X, xn, labels, mind=None, slots=None, track_changed: bool = False, rows=None,
               ub=None, lb=None, scatter: bool = False, count=None, oseed=None):
        """K2 on these centres (``X`` column-padded, 16-B rows).  ``rows`` (int64, device):
        assign the gathered batch X[rows] without materialising it (labels etc. logical, or
        at the rows themselves with ``scatter``).  ``ub`` / ``lb``: also write every point's
        distance to its nearest and second-nearest centre (the bounded E-step's bounds).
        ``count`` (int64 [1], device): assign only ``rows[:count]`` (a compacted batch).
        ``oseed`` (bf16, f32 [X rows]): every row's seed offset, from :func:`seed_offsets` --
        a gathered row then gets bitwise the scores (and label) of the full pass over ``X``."""
        if rows is not None:
            self._C.assign(X, self.pack, self.cn, xn, labels, mind, slots, self.Kpad, self.dpad,
                           track_changed, None, rows, ub, lb, scatter, count, oseed)
            return
        keys = None
        if 0 < X.shape[0] <= SPLIT_MAX_ROWS and ub is None:
            # small batches split the centre range across workgroups (assign16 grid.y);
            # the kernels leave the scratch all-ones again, so it is filled only once
            if self._keys is None or self._keys.numel() < X.shape[0]:
                self._keys = torch.full((X.shape[0],), -1, dtype=torch.int64, device=X.device)
            keys = self._keys
            if xn is not None and mind is None:   # the splits park each point's seed offset there
                mind = torch.empty(X.shape[0], dtype=torch.float32, device=X.device)
        self._C.assign(X, self.pack, self.cn, xn, labels, mind, slots, self.Kpad, self.dpad,
                       track_changed, keys, None, ub, lb, False, None, oseed)

    def seed_offsets(self, xn: torch.Tensor) -> "torch.Tensor | None":
        """Per-row seed offsets the full assign over rows with norms ``xn`` gives its bf16
        keys (its workgroup's, or the row's own; csrc/rows.hip seed_offsets); None for f32,
        whose scores carry no offset."""
        if self.dtype != torch.bfloat16:
            return None
        out = torch.empty(xn.numel(), dtype=torch.float32, device=xn.device)
        self._C.seed_offsets(xn, out, self._C.assign_block_rows(self.dt, self.dpad, self.Kpad))
        return out


def pack_centers(centers: torch.Tensor, D: int, dtype: torch.dtype, device):
    """A CentroidPack of ``centers`` for points with ``D`` (column-padded) features."""
    cen = torch.zeros((centers.shape[0], D), dtype=torch.float32, device=device)
    cen[:, : centers.shape[1]] = centers.to(device=device, dtype=torch.float32)
    return CentroidPack(cen.shape[0], D, dtype, device).load(cen)


def assign(X: torch.Tensor, centers: torch.Tensor, *, with_dist: bool = True,
           pack: "CentroidPack | None" = None):
    """Nearest centroid of every row: returns ``(labels int32, sqdist float32 or None)``.

    bf16 points are compared against bf16-quantised centroids (scores
    accumulated in fp32 on the matrix cores); f32 points use the exact-f32 MFMA.
    ``pack``: a CentroidPack of ``centers`` made earlier by :func:`pack_centers` for the
    same (padded) width, dtype and device (serving: pack once, assign many batches).
    """
    if not X.is_cuda or dpad_for(pad_columns(X[:1]).shape[1], X.dtype) == 0:
        return cpu.assign(X, centers.to(X.device), with_dist=with_dist)  # CPU, or D > 1024 on the GPU
    C = require()
    Xp = pad_columns(X)
    D = Xp.shape[1]
    if pack is not None and (pack.D, pack.dtype, pack.pack.device) == (D, Xp.dtype, Xp.device):
        pk = pack
    else:
        pk = pack_centers(centers, D, Xp.dtype, X.device)
    n = Xp.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    xn = mind = None
    if with_dist:
        xn = torch.empty(n, dtype=torch.float32, device=X.device)
        C.row_sqnorm(Xp, xn)
        mind = torch.empty(n, dtype=torch.float32, device=X.device)
    pk.assign(Xp, xn, labels, mind)
    return labels, mind


def transform(X: torch.Tensor, centers: torch.Tensor, *, squared: bool = False,
              pack: "CentroidPack | None" = None) -> torch.Tensor:
    """Distance of every row to every centre, ``[n, K]`` float32 (squared with ``squared``):
    on the GPU the MFMA transform kernel (csrc/transform.hip) on the assign kernel's packed
    centres -- the distances its argmin ranks; elsewhere the PyTorch reference."""
    if not X.is_cuda or dpad_for(pad_columns(X[:1]).shape[1], X.dtype) == 0:
        c = cpu.quantize_centers(centers.to(X.device), X.dtype)
        d = torch.cdist(X.to(torch.float32), c)
        return d * d if squared else d
    C = require()
    Xp = pad_columns(X)
    D = Xp.shape[1]
    if pack is not None and (pack.D, pack.dtype, pack.pack.device) == (D, Xp.dtype, Xp.device):
        pk = pack
    else:
        pk = pack_centers(centers, D, Xp.dtype, X.device)
    n = Xp.shape[0]
    xn = torch.empty(n, dtype=torch.float32, device=X.device)
    out = torch.empty((n, pk.K), dtype=torch.float32, device=X.device)
    if n:
        C.row_sqnorm(Xp, xn)
        C.transform(Xp, pk.pack, pk.cn, pk.K, pk.Kpad, pk.dpad, xn, out, squared)
    return out


TOPK_NATIVE_MAX = 32      # the top-m kernel's longest list (csrc/kernels.h TOPK_MAX)


def topk(X: torch.Tensor, centers: torch.Tensor, m: int, *, pack: "CentroidPack | None" = None):
    """The ``m`` nearest centres of every row: ``(idx int32 [n, m], d2 float32 [n, m])``, the
    squared distances ascending and equal ones by centre index -- the first ``m`` columns of a
    stable sort of ``transform(X, centers, squared=True)``, bit for bit.  On the GPU the fused
    MFMA kernel (csrc/topk.hip) keeps the ``m <= 32`` best in registers, so the ``[n, K]``
    matrix is never written; a longer list sorts the transform kernel's distances in row
    blocks of ~256 MB.  ``pack`` as in :func:`transform`.  Elsewhere the PyTorch reference."""
    m = int(m)
    K = centers.shape[0]
    if not 1 <= m <= K:
        raise ValueError(f"topk needs 1 <= m <= n_clusters ({K}), got m = {m}")
    if not X.is_cuda or dpad_for(pad_columns(X[:1]).shape[1], X.dtype) == 0:
        return cpu.topk(X, centers.to(X.device), m)  # CPU, or D > 1024 on the GPU
    C = require()
    Xp = pad_columns(X)
    D = Xp.shape[1]
    if pack is not None and (pack.D, pack.dtype, pack.pack.device) == (D, Xp.dtype, Xp.device):
        pk = pack
    else:
        pk = pack_centers(centers, D, Xp.dtype, X.device)
    n = Xp.shape[0]
    idx = torch.empty((n, m), dtype=torch.int32, device=X.device)
    d2 = torch.empty((n, m), dtype=torch.float32, device=X.device)
    if n == 0:
        return idx, d2
    if m <= TOPK_NATIVE_MAX:
        xn = torch.empty(n, dtype=torch.float32, device=X.device)
        C.row_sqnorm(Xp, xn)
        C.topk(Xp, pk.pack, pk.cn, pk.K, pk.Kpad, pk.dpad, xn, d2, idx)
        return idx, d2
    # distances, their sorted copy and int64 indices: 16 B per (row, centre)
    rows = max(1, (1 << 28) // (16 * K))
    for s in range(0, n, rows):
        d = transform(Xp[s : s + rows], centers, squared=True, pack=pk)
        v, i = torch.sort(d, dim=1, stable=True)
        d2[s : s + rows] = v[:, :m]
        idx[s : s + rows] = i[:, :m].to(torch.int32)
    return idx, d2


QUALITY_WORDS = cpu.QUALITY_WORDS   # csrc/kernels.h (the extension exports the same number)
QUALITY_BLOCK_ROWS = 1 << 22        # rows per top-2 pass of cluster_quality: 64 MB of (idx, d2) scratch


def quality_accumulate(table: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor, *, path: int = -1) -> torch.Tensor:
    """Add the per-cluster quality words of a top-1 / top-2 result (``idx`` int32, ``d2``
    float32, ``[n, 1 or 2]`` as :func:`topk` returns them) into ``table`` (int64
    ``[K, QUALITY_WORDS]``, zero before the first call): per label the exact digits of the
    sum of squared distances and the row count, the digits of the sum of distances, the
    non-finite rows, the fixed-point simplified-silhouette sum and the largest squared
    distance (csrc/quality.hip has the layout).  Integer atomics only, so the table does not
    depend on the order or the blocking of the rows.  GPU tensors run the native kernel
    (``path``: 0 forces its global-atomic form, 1 the LDS-private one, -1 the launcher's rule:
    tests and A/B runs), others the integer mirror :func:`mikmeans.ops.cpu.quality_table`."""
    if table.dim() != 2 or table.shape[1] != QUALITY_WORDS or table.dtype != torch.int64:
        raise ValueError(f"quality_accumulate needs an int64 [K, {QUALITY_WORDS}] table")
    if idx.is_cuda:
        C = require()
        assert C.QUALITY_WORDS == QUALITY_WORDS
        C.quality_accumulate(idx.contiguous(), d2.contiguous(), table, path)
        return table
    part = cpu.quality_table(idx, d2, table.shape[0])
    mx = torch.maximum(table[:, 17], part[:, 17])
    table += part
    table[:, 17] = mx
    return table


def _slot_value(W: torch.Tensor) -> torch.Tensor:
    """f64 value of summed digit words ``W[..., 0:7]`` (csrc/common.h slot_decode's order)."""
    v = torch.zeros(W.shape[:-1], dtype=torch.float64)
    for j in range(6, -1, -1):
        v = v + torch.ldexp(W[..., j].to(torch.float64), torch.tensor(32 * j - 64))
    return v


def _davies_bouldin(S: torch.Tensor, cq: torch.Tensor) -> float:
    """Mean over the clusters of max_{l != k} (S_k + S_l) / |c_k - c_l| in float64 (a zero
    separation counts as +inf, scikit-learn's convention), the centre distances in row
    blocks of <= 64 MB."""
    Kn = cq.shape[0]
    if Kn < 2:
        return float("nan")
    c = cq.to(torch.float64)
    s = S.to(device=c.device, dtype=torch.float64)
    rows = max(1, (1 << 26) // (8 * Kn))
    total = torch.zeros((), dtype=torch.float64, device=c.device)
    for i in range(0, Kn, rows):
        M = torch.cdist(c[i : i + rows], c, compute_mode="donot_use_mm_for_euclid_dist")
        R = (s[i : i + rows, None] + s[None, :]) / M
        R = torch.where(M > 0, R, torch.zeros_like(R))     # (the diagonal too)
        total = total + R.max(dim=1).values.sum()
    return float(total / Kn)


def quality_decode(table: torch.Tensor, centers: torch.Tensor, dtype: torch.dtype = torch.float32) -> dict:
    """The cluster report of a quality table: float64 arithmetic in a fixed order on the host
    (the centre distances of the Davies-Bouldin index on the centres' device).

    Per cluster (CPU tensors ``[K]``): ``counts`` (int64, rows with a finite distance),
    ``cluster_inertia`` (sum a^2), ``mean_distance`` (sum a / n_k), ``rms_distance``,
    ``radius`` (the largest a), ``cluster_silhouette`` (mean simplified silhouette
    1 - a / b over the cluster's rows) and ``n_nonfinite`` (int64, rows left out because their
    distance is NaN or infinite); empty clusters get NaN means and radius 0.  Totals:
    ``n_samples``, ``inertia`` (decoded from the digit words summed over the labels as
    integers), ``silhouette`` (NaN for K = 1), ``balance`` and ``davies_bouldin`` (S =
    ``mean_distance``, M = the distance between the centres as the kernels rank them; NaN
    with fewer than two non-empty clusters)."""
    from ..utils import metrics as mmetrics

    T = table.detach().to("cpu")
    K = T.shape[0]
    counts = T[:, 7].clone()
    nk = counts.to(torch.float64)
    nan = torch.full((K,), float("nan"), dtype=torch.float64)
    empty = counts == 0
    inertia_k = _slot_value(T[:, 0:7])
    suma = _slot_value(T[:, 8:15])
    mean_d = torch.where(empty, nan, suma / nk)
    rms = torch.where(empty, nan, (inertia_k / nk).sqrt())
    sil_k = torch.where(empty | (K == 1), nan, T[:, 16].to(torch.float64) / nk / 2147483648.0)
    radius = T[:, 17].to(torch.int32).view(torch.float32).to(torch.float64).sqrt()
    n = int(counts.sum())
    sil = float(T[:, 16].sum()) / n / 2147483648.0 if (K > 1 and n > 0) else float("nan")
    full = (~empty).nonzero().flatten()
    cq = cpu.quantize_centers(centers, dtype)
    db = _davies_bouldin(mean_d[full], cq[full.to(cq.device)])
    return {
        "counts": counts, "cluster_inertia": inertia_k, "mean_distance": mean_d, "rms_distance": rms,
        "radius": radius, "cluster_silhouette": sil_k, "n_nonfinite": T[:, 15].clone(),
        "n_samples": n, "inertia": float(_slot_value(T[:, 0:7].sum(0))), "silhouette": sil,
        "davies_bouldin": db, "balance": mmetrics.balance([int(c) for c in counts.tolist()]),
    }


def quality_rows(table: torch.Tensor, X: torch.Tensor, centers: torch.Tensor, *,
                 pack: "CentroidPack | None" = None, block_rows: int | None = None) -> torch.Tensor:
    """Accumulate the rows of ``X`` into ``table``: :func:`topk` with min(2, K) then
    :func:`quality_accumulate`, in row blocks (``block_rows``, default 2^22), so the top-2
    scratch stays bounded at any n.  The table does not depend on the block size."""
    K = centers.shape[0]
    block = int(block_rows) if block_rows else QUALITY_BLOCK_ROWS
    if X.is_cuda and pack is None and X.shape[0] > block:   # pack the centres once for all blocks
        X = pad_columns(X)
        if dpad_for(X.shape[1], X.dtype):
            pack = pack_centers(centers, X.shape[1], X.dtype, X.device)
    for s in range(0, X.shape[0], block):
        idx, d2 = topk(X[s : s + block], centers, min(2, K), pack=pack)
        quality_accumulate(table, idx, d2)
    return table


def cluster_quality(X: torch.Tensor, centers: torch.Tensor, *, pack: "CentroidPack | None" = None,
                    block_rows: int | None = None):
    """Per-cluster quality of the rows of ``X`` under ``centers``: ``(report, table)``, the
    report :func:`quality_decode`'s dict and the table the int64 ``[K, QUALITY_WORDS]``
    reduction it was decoded from (on ``X``'s device)."""
    table = torch.zeros((centers.shape[0], QUALITY_WORDS), dtype=torch.int64, device=X.device)
    quality_rows(table, X, centers, pack=pack, block_rows=block_rows)
    return quality_decode(table, centers, X.dtype), table


EXEMPLAR_MAX = cpu.EXEMPLAR_MAX     # csrc/kernels.h (the extension exports the same number)
EXEMPLAR_BLOCK_ROWS = 1 << 22       # rows per top-1 pass of cluster_exemplars: 32 MB of (idx, d2) scratch


def exemplar_new(K: int, m: int, device=None) -> torch.Tensor:
    """An empty exemplar table: int64 ``[K, m]``, every word all ones."""
    m = int(m)
    if not 1 <= m <= EXEMPLAR_MAX:
        raise ValueError(f"cluster_exemplars needs 1 <= m <= {EXEMPLAR_MAX}, got m = {m}")
    return torch.full((int(K), m), cpu.EXEMPLAR_EMPTY, dtype=torch.int64, device=device)


def exemplar_accumulate(table: torch.Tensor, idx: torch.Tensor, d2: torch.Tensor, *, row0: int = 0,
                        farthest: bool = False, path: int = -1) -> torch.Tensor:
    """Min-insert the rows of a top-m result (``idx`` int32, ``d2`` float32, ``[n, m_topk]`` as
    :func:`topk` returns them; column 0 is read) into ``table`` (int64 ``[K, m]``, all ones
    before the first call, :func:`exemplar_new`): slot j of cluster k ends as the (j+1)-th
    smallest key ``hi << 32 | (row0 + row)`` of the cluster's rows, ``hi`` the bit pattern of the
    squared distance (``farthest``: 0x7F7FFFFF minus it), so a list is the cluster's ``m``
    nearest (farthest) rows, equal distances by the lower row (csrc/exemplars.hip has the
    layout).  Rows with a label outside ``[0, K)`` or a non-finite distance are in no list.
    64-bit integer atomic min only, so the table does not depend on the order or the blocking of
    the rows.  GPU tensors run the native kernel (``path``: 0 forces its global-atomic form, 1
    the LDS-private one, -1 the launcher's rule: tests and A/B runs), others the integer mirror
    :func:`mikmeans.ops.cpu.exemplar_table` and :func:`mikmeans.ops.cpu.exemplar_merge`."""
    if table.dim() != 2 or not 1 <= table.shape[1] <= EXEMPLAR_MAX or table.dtype != torch.int64:
        raise ValueError(f"exemplar_accumulate needs an int64 [K, m] table with 1 <= m <= {EXEMPLAR_MAX}")
    row0 = int(row0)
    if row0 < 0 or row0 + idx.shape[0] > 1 << 32:
        raise ValueError("exemplar_accumulate takes row indices below 2^32 (row0 + n): split the rows over calls")
    if idx.is_cuda:
        C = require()
        assert C.EXEMPLAR_MAX == EXEMPLAR_MAX
        C.exemplar_accumulate(idx.contiguous(), d2.contiguous(), table, row0, bool(farthest), path)
        return table
    part = cpu.exemplar_table(idx, d2, table.shape[0], table.shape[1], row0, farthest)
    table.copy_(cpu.exemplar_merge(table, part))
    return table


def exemplar_decode(table: torch.Tensor, *, farthest: bool = False, row_start: int = 0):
    """``(rows int64 [K, m], d2 float32 [K, m])`` of an exemplar table: each slot's row index
    (plus ``row_start``) and squared distance, -1 and NaN for the empty slots."""
    empty = table == cpu.EXEMPLAR_EMPTY
    rows = torch.where(empty, -1, (table & 0xFFFFFFFF) + int(row_start))
    hi = torch.where(empty, 0, table >> 32)
    bits = (0x7F7FFFFF - hi) if farthest else hi
    d2 = bits.to(torch.int32).view(torch.float32)
    return rows, torch.where(empty, float("nan"), d2)


def exemplar_rows(table: torch.Tensor, X: torch.Tensor, centers: torch.Tensor, *, row0: int = 0,
                  farthest: bool = False, pack: "CentroidPack | None" = None,
                  block_rows: int | None = None) -> torch.Tensor:
    """Accumulate the rows of ``X`` (row i counted as ``row0 + i``) into ``table``: :func:`topk`
    with m = 1 then :func:`exemplar_accumulate`, in row blocks (``block_rows``, default 2^22), so
    the top-1 scratch stays bounded at any n.  The table does not depend on the block size."""
    block = int(block_rows) if block_rows else EXEMPLAR_BLOCK_ROWS
    if int(row0) < 0 or int(row0) + X.shape[0] > 1 << 32:
        raise ValueError("cluster_exemplars takes fewer than 2^32 rows in one call")
    if X.is_cuda and pack is None and X.shape[0] > block:   # pack the centres once for all blocks
        X = pad_columns(X)
        if dpad_for(X.shape[1], X.dtype):
            pack = pack_centers(centers, X.shape[1], X.dtype, X.device)
    for s in range(0, X.shape[0], block):
        idx, d2 = topk(X[s : s + block], centers, 1, pack=pack)
        exemplar_accumulate(table, idx, d2, row0=int(row0) + s, farthest=farthest)
    return table


def cluster_exemplars(X: torch.Tensor, centers: torch.Tensor, m: int, *, farthest: bool = False,
                      pack: "CentroidPack | None" = None, block_rows: int | None = None):
    """For every centre the ``m`` rows of ``X`` assigned to it that lie nearest it (``farthest``:
    farthest from it): ``(rows int64 [K, m], d2 float32 [K, m], table)``, the squared distances
    in list order, -1 / NaN where a cluster has fewer than ``m`` rows, and the int64 ``[K, m]``
    table both were decoded from (on ``X``'s device)."""
    table = exemplar_new(centers.shape[0], m, X.device)
    exemplar_rows(table, X, centers, farthest=farthest, pack=pack, block_rows=block_rows)
    rows, d2 = exemplar_decode(table, farthest=farthest)
    return rows, d2, table


QUANTILE_MAX_Q = cpu.QUANTILE_MAX_Q     # csrc/kernels.h (the extension exports the same number)
QUANTILE_BINS = cpu.QUANTILE_BINS
QUANTILE_PASSES = cpu.QUANTILE_PASSES
QUANTILE_BLOCK_ROWS = 1 << 22           # rows per top-1 pass of cluster_quantiles


def quantile_levels(q) -> list[float]:
    """``q`` (a number or a sequence of them) as a list of 1..QUANTILE_MAX_Q floats in [0, 1]."""
    try:
        qs = torch.as_tensor(q, dtype=torch.float64).reshape(-1).tolist()
    except (TypeError, ValueError, RuntimeError) as e:
        raise ValueError(f"cluster_quantiles needs numbers in [0, 1], got {q!r}") from e
    if not 1 <= len(qs) <= QUANTILE_MAX_Q:
        raise ValueError(f"cluster_quantiles takes 1 to {QUANTILE_MAX_Q} quantiles in one call, got {len(qs)}")
    for v in qs:
        if not 0.0 <= v <= 1.0:                      # (NaN fails both comparisons)
            raise ValueError(f"cluster_quantiles needs every q finite and in [0, 1], got {v}")
    return qs


def quantile_state(K: int, Q: int, device=None):
    """The radix select's state before pass 0: ``(prefix int32 [K, Q], rank int64 [K, Q], counts
    int64 [K])``, all zero."""
    K, Q = int(K), int(Q)
    if not 1 <= Q <= QUANTILE_MAX_Q:
        raise ValueError(f"cluster_quantiles takes 1 to {QUANTILE_MAX_Q} quantiles in one call, got {Q}")
    return (torch.zeros((K, Q), dtype=torch.int32, device=device), torch.zeros((K, Q), dtype=torch.int64, device=device),
            torch.zeros(K, dtype=torch.int64, device=device))


def quantile_hist(idx: torch.Tensor, d2: torch.Tensor, K: int, prefix: torch.Tensor, pass_: int, *,
                  table: torch.Tensor | None = None, path: int = -1, agg: int = -1) -> torch.Tensor:
    """Add the rows of a top-m result (``idx`` int32, ``d2`` float32, ``[n, m_topk]`` as
    :func:`topk` returns them; column 0 is read) into pass ``pass_``'s digit histogram ``table``
    (int64 ``[K, 256]`` in pass 0, ``[K, Q, 256]`` in passes 1..3; a zero one is made when none is
    given) and return it: in pass 0 a row adds one to ``(k, bits >> 24)``, later to
    ``(k, j, (bits >> s) & 255)`` for every j whose ``prefix`` (int32 ``[K, Q]``) shares its bits
    above ``s + 8`` (csrc/quantiles.hip has the passes).  Rows with a label outside ``[0, K)`` or a
    non-finite distance count nowhere.  64-bit integer atomic add only, so the table does not
    depend on the order or the blocking of the rows.  GPU tensors run the native kernel
    (``path``: 0 forces its global-atomic form, 1 the LDS-private one, 2 the banded LDS one, -1
    the launcher's rule; ``agg``: the wave-aggregation rounds, -1 the form's constant: tests and
    A/B runs), others
    the integer mirror :func:`mikmeans.ops.cpu.quantile_hist`."""
    K, pass_ = int(K), int(pass_)
    if not 0 <= pass_ < QUANTILE_PASSES:
        raise ValueError(f"quantile_hist needs a pass in 0..3, got {pass_}")
    Q = int(prefix.shape[1])
    shape = (K, QUANTILE_BINS) if pass_ == 0 else (K, Q, QUANTILE_BINS)
    if table is None:
        table = torch.zeros(shape, dtype=torch.int64, device=idx.device)
    if tuple(table.shape) != shape or table.dtype != torch.int64:
        raise ValueError(f"quantile_hist needs an int64 {list(shape)} table in pass {pass_}")
    if idx.is_cuda:
        C = require()
        assert C.QUANTILE_MAX_Q == QUANTILE_MAX_Q and C.QUANTILE_BINS == QUANTILE_BINS
        C.quantile_hist(idx.contiguous(), d2.contiguous(), table, prefix if pass_ else None, pass_, path, agg)
        return table
    table += cpu.quantile_hist(idx, d2, K, prefix, pass_)
    return table


def quantile_select(table: torch.Tensor, q: torch.Tensor, prefix: torch.Tensor, rank: torch.Tensor,
                    counts: torch.Tensor, pass_: int) -> None:
    """One select step on pass ``pass_``'s summed histogram, in place: per (cluster, q) the
    smallest bin whose running count exceeds the remaining rank joins ``prefix`` at shift
    ``24 - 8 * pass_`` and ``rank`` drops by the count below it; pass 0 first writes ``counts`` =
    n_k and derives the rank r = clamp(ceil(q * n_k) - 1, 0, n_k - 1) from ``q`` (float64
    ``[Q]``).  GPU tensors run the native kernel, others :func:`mikmeans.ops.cpu.quantile_select`."""
    if table.is_cuda:
        require().quantile_select(table, q, prefix, rank, counts, int(pass_))
        return
    P, R, n = cpu.quantile_select(table, q, prefix, rank, pass_)
    prefix.copy_(P)
    rank.copy_(R)
    if n is not None:
        counts.copy_(n)


def quantile_top1(X: torch.Tensor, centers: torch.Tensor, *, pack: "CentroidPack | None" = None,
                  block_rows: int | None = None) -> list:
    """The top-1 ``(idx, d2)`` of every row of ``X``, a list of one pair per row block
    (``block_rows``, default 2^22): the 8 B per row that the four histogram passes of
    :func:`quantile_passes` read."""
    block = int(block_rows) if block_rows else QUANTILE_BLOCK_ROWS
    if X.is_cuda and pack is None and X.shape[0] > block:   # pack the centres once for all blocks
        X = pad_columns(X)
        if dpad_for(X.shape[1], X.dtype):
            pack = pack_centers(centers, X.shape[1], X.dtype, X.device)
    return [topk(X[s : s + block], centers, 1, pack=pack) for s in range(0, X.shape[0], block)]


def quantile_passes(chunks, K: int, q, device=None, *, reduce=None):
    """The radix select over kept top-1 output (``chunks``: ``(idx, d2)`` pairs, fewer than 2^32
    rows each): ``(d2_values float32 [K, Q], counts int64 [K])``, per cluster and ``q`` the
    squared distance at sorted position clamp(ceil(q * n_k) - 1, 0, n_k - 1) of the cluster's
    rows, NaN for a cluster without rows.  ``reduce`` (a callable, in place) is applied to each
    pass's histogram before its select: a multi-rank job's all-reduce.  No host read between
    the passes."""
    qs = quantile_levels(q)
    qt = torch.tensor(qs, dtype=torch.float64, device=device)
    prefix, rank, counts = quantile_state(K, len(qs), device)
    for p in range(QUANTILE_PASSES):
        shape = (int(K), QUANTILE_BINS) if p == 0 else (int(K), len(qs), QUANTILE_BINS)
        table = torch.zeros(shape, dtype=torch.int64, device=device)
        for idx, d2 in chunks:
            quantile_hist(idx, d2, K, prefix, p, table=table)
        if reduce is not None:
            reduce(table)
        quantile_select(table, qt, prefix, rank, counts, p)
    values = torch.where((counts > 0)[:, None], prefix.view(torch.float32), float("nan"))
    return values, counts


def cluster_quantiles(X: torch.Tensor, centers: torch.Tensor, q, *, pack: "CentroidPack | None" = None,
                      block_rows: int | None = None, reduce=None):
    """Exact per-cluster quantiles of the squared distances of the rows of ``X`` to their nearest
    centre: ``(d2_values float32 [K, Q], counts int64 [K])``.  One top-1 pass in row blocks, its
    ``(idx, d2)`` kept (8 B per row), then four histogram passes over it (:func:`quantile_passes`);
    no sort, and every value is a real row's squared distance bit for bit."""
    quantile_levels(q)
    chunks = quantile_top1(X, centers, pack=pack, block_rows=block_rows)
    return quantile_passes(chunks, centers.shape[0], q, X.device, reduce=reduce)


def max_abs(X: torch.Tensor) -> float:
    """max |x| without materialising |X| (one host read)."""
    if X.numel() == 0:
        return 0.0
    mn, mx = torch.aminmax(X)
    return max(abs(float(mn)), abs(float(mx)))


def _native_colstats_ok(X: torch.Tensor) -> bool:
    v = 16 // X.element_size()
    return (X.is_cuda and X.dtype in (torch.float32, torch.bfloat16) and X.dim() == 2 and X.stride(1) == 1
            and X.shape[1] % v == 0 and (X.shape[0] <= 1 or X.stride(0) % v == 0)
            and X.data_ptr() % 16 == 0)


def col_max_abs(X: torch.Tensor) -> torch.Tensor:
    """Per-column max |x| as float64 ``[D]`` (no |X| temporary)."""
    return col_stats(X, stats=False).absmax


class ColStats:
    """Per-column statistics of one streaming pass (csrc/finalize.hip col_absmax):
    ``absmax`` (f64 [D]); with ``stats``: ``sumabs``, ``sum``, ``sumsq`` (f64), ``nnz``
    (int64, nonzero values) and ``lowbit`` (int32: every value is an integer multiple of
    2^lowbit; LOWBIT_NONE for an all-zero column).  Statistics of row blocks merge with
    :meth:`merge` (streamed shards)."""

    LOWBIT_NONE = 2**31 - 1

    def __init__(self, absmax, sumabs=None, nnz=None, lowbit=None, sum=None, sumsq=None):
        self.absmax, self.sumabs, self.nnz, self.lowbit = absmax, sumabs, nnz, lowbit
        self.sum, self.sumsq = sum, sumsq

    @property
    def full(self) -> bool:
        return self.sumabs is not None

    def merge(self, other: "ColStats") -> "ColStats":
        if not (self.full and other.full):
            return ColStats(torch.maximum(self.absmax, other.absmax))
        return ColStats(torch.maximum(self.absmax, other.absmax), self.sumabs + other.sumabs,
                        self.nnz + other.nnz, torch.minimum(self.lowbit, other.lowbit),
                        self.sum + other.sum, self.sumsq + other.sumsq)

    @staticmethod
    def empty(D: int, device, full: bool = True) -> "ColStats":
        z = torch.zeros(D, dtype=torch.float64, device=device)
        if not full:
            return ColStats(z)
        return ColStats(z, z.clone(), torch.zeros(D, dtype=torch.int64, device=device),
                        torch.full((D,), ColStats.LOWBIT_NONE, dtype=torch.int32, device=device),
                        z.clone(), z.clone())


def _lowbit_torch(Xb: torch.Tensor) -> torch.Tensor:
    """Exponent of the lowest set bit of each nonzero finite value (f32 semantics)."""
    b = Xb.to(torch.float32).contiguous().view(torch.int32).long() & 0x7FFFFFFF
    e = b >> 23
    m = b & 0x7FFFFF
    sig = torch.where(e == 0, m, m | 0x800000)
    tz = ((sig & -sig).clamp_min(1).double().log2()).long()
    lb = torch.where(e == 0, -149 + tz, e - 150 + tz)
    return torch.where((b == 0) | (e == 255), torch.full_like(lb, ColStats.LOWBIT_NONE), lb)


def fused_norms_ok(X: torch.Tensor) -> bool:
    """Whether :func:`col_stats` can also write the row norms (a row of <= 64 16-B pieces)."""
    return _native_colstats_ok(X) and X.shape[1] <= 64 * (16 // X.element_size())


def col_stats(X: torch.Tensor, stats: bool = True, xn: torch.Tensor | None = None) -> ColStats:
    """One pass over ``X``: per-column max |x| and, with ``stats``, sum |x|, sum x, sum x^2,
    the nonzero count and the lowest-bit exponent (native kernel on the GPU, whose f64 sums
    are per-block partials summed in a fixed order: bitwise the same on every launch; torch
    elsewhere).  ``xn`` (GPU, :func:`fused_norms_ok`): also every row's |x|^2 into it, bitwise
    :func:`row_sqnorm`'s -- the fit's setup then reads X once."""
    D = X.shape[1]
    if X.shape[0] == 0:
        return ColStats.empty(D, X.device, stats)
    if xn is not None and not fused_norms_ok(X):
        raise ValueError("col_stats: fused row norms need a native-layout GPU X of <= 64 pieces per row")
    if _native_colstats_ok(X):
        out = torch.zeros(D, dtype=torch.int32, device=X.device)
        if not stats:
            require().col_absmax(X, out, None, None, None, xn)
            return ColStats(out.view(torch.float32).double())
        fs = torch.zeros((3, D), dtype=torch.float64, device=X.device)
        nz = torch.zeros(D, dtype=torch.int64, device=X.device)
        lb = torch.full((D,), ColStats.LOWBIT_NONE, dtype=torch.int32, device=X.device)
        require().col_absmax(X, out, fs, nz, lb, xn)
        return ColStats(out.view(torch.float32).double(), fs[0], nz, lb, fs[1], fs[2])
    mn, mx = torch.aminmax(X, dim=0)
    m = torch.maximum(mn.double().abs(), mx.double().abs())
    if not stats:
        return ColStats(m)
    st = ColStats.empty(D, X.device)
    st.absmax = m
    lb = st.lowbit.long()
    for i in range(0, X.shape[0], 1 << 16):
        xb = X[i : i + (1 << 16)].to(torch.float64)
        st.sumabs += xb.abs().sum(0)
        st.sum += xb.sum(0)
        st.sumsq += (xb * xb).sum(0)
        st.nnz += (xb != 0).sum(0)
        lb = torch.minimum(lb, _lowbit_torch(X[i : i + (1 << 16)]).amin(0))
    st.lowbit = lb.to(torch.int32)
    return st


# A column whose values do not all sit on the hi pass's grid (2^-col_exp) and whose max |x|
# exceeds WIDE_RATIO x the mean of its NONZERO |x| gets the residual (lo) M-step pass: its
# contributions are then exact to 2^-41 (not 2^-21) of the column maximum, so one outlier no
# longer coarsens every other point's contribution (csrc/update.hip UPD_RESID).  Columns the
# hi grid represents exactly (one-hot, small integers) and sparse columns never need it.
WIDE_RATIO = 256.0


def fixed_exps(X: torch.Tensor, weights: torch.Tensor | None = None, comm=None, bound=None):
    """Fixed-point exponents of the M-step accumulators (csrc/update.hip).

    Returns ``(col_exp, cnt_exp)``: an int32 device tensor ``[D]`` such that every
    contribution ``|x[:, d] * w| * 2^col_exp[d] <= 2^20``, and the exponent of the
    weighted counts.  ``bound`` (per-column float64 ``[D]``) overrides the data's
    column maxima; with ``comm`` the maxima are all-reduced so every rank uses the
    same scale (exact, world-size independent sums)."""
    sc = mstep_scales(X, weights, comm=comm, bound=bound, wide_ratio=0)
    return sc.col_exp, sc.cnt_exp


class MStepScales:
    """Fixed-point scales of one fit's M-step plus its wide-range columns.

    ``col_exp``/``cnt_exp`` as in :func:`fixed_exps`; ``wide_cols`` (int32 ``[nw]``) are
    the columns with max |x| > ``wide_ratio`` x mean |x|, ``wide_exps`` their lo-pass
    exponents (``col_exp + 20``) and ``col_exp2`` the kernel's per-column form (-1000
    = no lo pass)."""

    def __init__(self, col_exp, cnt_exp, wide_cols, device):
        self.col_exp, self.cnt_exp = col_exp, cnt_exp
        wc = sorted(int(c) for c in wide_cols)
        ce = col_exp.cpu()
        self.wide_cols = torch.tensor(wc, dtype=torch.int32, device=device)
        self.wide_exps = torch.tensor([int(ce[c]) + 20 for c in wc], dtype=torch.int32, device=device)
        e2 = torch.full_like(ce, -1000)
        for c in wc:
            e2[c] = int(ce[c]) + 20
        self.col_exp2 = e2.to(device)
        self.nw = len(wc)


def mstep_scales(X: torch.Tensor, weights: torch.Tensor | None = None, comm=None, bound=None,
                 n_global: int | None = None, wide_ratio: float | None = None,
                 stats: ColStats | None = None) -> MStepScales:
    """Scales of the fixed-point M-step (global over ranks) and the wide-range columns.
    ``stats``: this rank's column statistics when already computed (streamed shards)."""
    C = require()
    ratio = WIDE_RATIO if wide_ratio is None else float(wide_ratio)
    want = bound is None and ratio > 0
    st = None
    if bound is None:
        st = stats if stats is not None else col_stats(X, stats=want)
        m = st.absmax.to(device=X.device, dtype=torch.float64).clone()
    else:
        m = bound.to(device=X.device, dtype=torch.float64)
    wm = torch.zeros(1, dtype=torch.float64, device=X.device)
    if weights is not None and weights.numel():
        wm[0] = max_abs(weights)
    want = want and st is not None and st.sumabs is not None
    if want:
        sa = st.sumabs.to(device=X.device, dtype=torch.float64).clone()
        nz = st.nnz.to(device=X.device, dtype=torch.float64)
        lb = st.lowbit.to(device=X.device, dtype=torch.float64)
    if comm is not None:
        comm.allreduce_max_(m)
        comm.allreduce_max_(wm)
        if want:
            comm.allreduce_(sa)
            comm.allreduce_(nz)
            lb = -lb
            comm.allreduce_max_(lb)        # global min of the lowest-bit exponents
            lb = -lb
    w = float(wm.item()) if weights is not None else 1.0
    mh = m.cpu()
    exps = [C.fixed_exp(v * w) for v in mh.tolist()]
    col_exp = torch.tensor(exps, dtype=torch.int32, device=X.device)
    wide = []
    if want:
        mean_nz = (sa / nz.clamp_min(1)).cpu()
        lbh = lb.cpu()
        for d in range(len(exps)):
            # weighted contributions x*w are never assumed to sit on the grid
            exact = weights is None and lbh[d] + exps[d] >= 0
            if (mh[d] > 0 and not exact and mh[d] > ratio * mean_nz[d]
                    and exps[d] + 20 <= 126):  # the lo scale must stay a normal float
                wide.append(d)
    return MStepScales(col_exp, C.fixed_exp(w) if weights is not None else 0, wide, X.device)


def add_wide_lo(packed: torch.Tensor, K: int, D: int, sc: MStepScales) -> None:
    """After the all-reduce: add the wide columns' lo sums (message tail) onto their hi
    sums -- one f64 rounding of two exact integer-valued totals, so world-size invariant."""
    if not sc.nw:
        return
    KD = K * D
    lo = packed[KD + K + 2 : KD + K + 2 + K * sc.nw].view(K, sc.nw)
    pv = packed[:KD].view(K, D)
    idx = sc.wide_cols.long()
    pv.index_copy_(1, idx, pv.index_select(1, idx) + lo)


def cluster_sums(X: torch.Tensor, labels: torch.Tensor, K: int, weights: torch.Tensor | None = None):
    """Per-cluster f64 sums ``[K, D]`` and counts ``[K]`` (weighted when ``weights``)."""
    if not X.is_cuda:
        return cpu.cluster_sums(X, labels, K, weights)
    C = require()
    Xp = pad_columns(X)
    n, D = Xp.shape
    dt = dtype_code(Xp.dtype)
    nch = C.update_n_chunks(dt, K, D, n, weights is not None)
    slab = torch.empty(nch * K * D, dtype=torch.int64, device=X.device)
    cnt = torch.empty(nch * K, dtype=torch.int64, device=X.device)
    lab = labels.to(torch.int32).contiguous()
    w = weights.to(torch.float32).contiguous() if weights is not None else None
    sc = mstep_scales(Xp, w, n_global=n)
    if sc.nw and C.update_slice_width(dt, K, D, w is not None) == 0:
        sc = MStepScales(sc.col_exp, sc.cnt_exp, [], X.device)  # global-atomic fallback: no lo pass
    packed = torch.zeros(K * D + K + 2 + K * sc.nw, dtype=torch.float64, device=X.device)
    C.update(Xp, lab, K, slab, cnt, nch, w, sc.col_exp, sc.cnt_exp, False)
    C.reduce(slab, cnt, nch, K, D, None, packed, sc.col_exp, sc.cnt_exp)
    if sc.nw:
        C.update(Xp, lab, K, slab, cnt, nch, w, sc.col_exp, sc.cnt_exp, False, col_exp2=sc.col_exp2)
        C.reduce_cols(slab, nch, K, D, sc.wide_cols, sc.wide_exps, packed[K * D + K + 2 :])
        add_wide_lo(packed, K, D, sc)
    sums = packed[: K * D].view(K, D)[:, : X.shape[1]]
    return sums, packed[K * D : K * D + K]
