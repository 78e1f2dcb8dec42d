"""Per-cluster analytics: the folds over the top-k output and their decodes.

Each of the three features has one shape: :func:`mikmeans.ops.topk_blocks` gives every row's
nearest (and second-nearest) centre in row blocks, a fold (csrc/quality.hip,
csrc/exemplars.hip, csrc/quantiles.hip on the frame of csrc/fold.h; the integer mirrors of
:mod:`mikmeans.ops.cpu` elsewhere) adds the ``(idx, d2)`` columns into a per-cluster integer
table with integer atomics only, the table is reduced over the ranks and decoded on the host.

* :func:`cluster_quality`    sizes, inertia, mean / rms distance, radius, silhouette, Davies-Bouldin
* :func:`cluster_exemplars`  the m rows nearest (farthest from) every centre
* :func:`cluster_quantiles`  exact per-cluster distance quantiles by radix select
"""
from __future__ import annotations

import torch

from . import TOPK_BLOCK_ROWS, CentroidPack, cpu, topk_blocks
from .native import require

# Everything here is re-exported by mikmeans.ops: callers say ops.NAME.
__all__ = [
    "QUALITY_WORDS", "QUALITY_BLOCK_ROWS", "quality_accumulate", "quality_decode", "quality_rows", "cluster_quality",
    "EXEMPLAR_MAX", "EXEMPLAR_BLOCK_ROWS", "exemplar_new", "exemplar_accumulate", "exemplar_decode", "exemplar_rows",
    "cluster_exemplars",
    "QUANTILE_MAX_Q", "QUANTILE_BINS", "QUANTILE_PASSES", "QUANTILE_BLOCK_ROWS", "quantile_levels", "quantile_state",
    "quantile_hist", "quantile_select", "quantile_top1", "quantile_passes", "cluster_quantiles",
]

# The three folds share one block size (mikmeans.ops.topk_blocks); scripts read it by feature.
QUALITY_BLOCK_ROWS = EXEMPLAR_BLOCK_ROWS = QUANTILE_BLOCK_ROWS = TOPK_BLOCK_ROWS

QUALITY_WORDS = cpu.QUALITY_WORDS   # csrc/kernels.h (the extension exports the same number)


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
    for _, idx, d2 in topk_blocks(X, centers, min(2, centers.shape[0]), pack=pack, block_rows=block_rows):
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
    if int(row0) < 0 or int(row0) + X.shape[0] > 1 << 32:
        raise ValueError("cluster_exemplars takes fewer than 2^32 rows in one call")
    for s, idx, d2 in topk_blocks(X, centers, 1, pack=pack, block_rows=block_rows):
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
    return [(idx, d2) for _, idx, d2 in topk_blocks(X, centers, 1, pack=pack, block_rows=block_rows)]


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
