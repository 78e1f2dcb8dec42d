"""The fitted clusters as an inverted-file (IVF-Flat) index: nearest-row search through the lists.

* :func:`partition`     rows grouped by label on the device (csrc/ivf.hip: count, scan, scatter)
* :func:`index_build`   every row's list (:func:`mikmeans.ops.topk` with m = 1), the partition and the
  rows packed list after list as if they were centres
* :func:`index_add` / :func:`index_remove`  a new index with rows added or taken out: only the new
  rows meet the centres, the rows that stay are copied from the old pack (csrc/ivf.hip: the repack)
* :func:`index_search`  the ``nprobe`` nearest centres of every query, the scan of their lists and
  the per-query merge: sorted ``(d2 bits << 32 | row)`` keys
* :func:`index_range`   every row of those lists within a radius of the query (csrc/range.hip: a count
  pass, a cumulative sum and a fill pass): ``(lims, keys)``, a variable number of keys per query
* :func:`index_search_deep`  :func:`index_search` for up to 2048 rows a query: a radix select over the
  ``d2`` bits (csrc/deep.hip: :func:`index_hist` / :func:`index_select`) finds every query's m-th
  distance, the range passes collect the rows under it
* :func:`index_decode`  keys to ``(rows, squared distances)``

GPU tensors of up to 1024 features run the native kernels; CPU tensors and wider rows run the
mirrors of :mod:`mikmeans.ops.cpu`, which keep the same lists and the same tensors (the rows in
natural layout instead of the fragment pack).
"""
from __future__ import annotations

import torch

from . import TOPK_NATIVE_MAX, cpu, pad_columns, row_sqnorm, topk, topk_blocks
from .native import dpad_for, dtype_code, require

__all__ = ["PARTITION_MAX_K", "IVF_EMPTY_KEY", "INDEX_MAX_M", "INDEX_SCAN_KEYS", "partition", "RowIndex",
           "index_tiles", "pair_items", "index_build", "index_add", "index_remove", "index_search", "index_range",
           "index_decode", "INDEX_DEEP_MAX_M", "INDEX_DEEP_OVERSHOOT", "deep_block_queries", "index_hist",
           "index_select", "index_search_deep"]

PARTITION_MAX_K = cpu.PARTITION_MAX_K   # csrc/kernels.h (the extension exports the same number)
IVF_EMPTY_KEY = cpu.IVF_EMPTY_KEY       # a result slot without a row: behind every key
INDEX_MAX_M = TOPK_NATIVE_MAX           # the scan kernel's longest list (TOPK_MAX)
INDEX_SCAN_KEYS = 1 << 27               # keys (8 B each) one scan launch may write: queries go in blocks
INDEX_DEEP_MAX_M = cpu.INDEX_DEEP_MAX_M  # the longest deep-search result (csrc/kernels.h IVF_DEEP_MAX_M)
# A deep search stops selecting digits once its radius lets through at most this many times the
# rows wanted, summed over the block: one more histogram walk against fill and sort volume
# (docs/SEARCH_DEEP.md has the measurement).  The result does not depend on it.
INDEX_DEEP_OVERSHOOT = 2
QUANTILE_BINS = cpu.QUANTILE_BINS


def partition(labels: torch.Tensor, K: int, *, want_pos: bool = False):
    """Stable partition of the rows by label: ``(order int64 [n], offsets int64 [K + 1])``.
    ``order[:offsets[K]]`` holds the rows whose label lies in ``[0, K)``, label after label and
    ascending within a label -- ``torch.sort(labels[valid], stable=True)``'s permutation -- its tail
    is -1, and ``offsets`` is the cumulative bincount.  ``want_pos``: also ``rpos`` (int64 [n]),
    every row's position in ``order`` (-1 for a row in no list).  On the GPU the native count /
    scan / scatter passes (no atomic decides a position, no host read) for
    ``K <= PARTITION_MAX_K``; beyond that, and for CPU tensors, a stable ``torch.sort``."""
    K = int(K)
    if labels.dim() != 1:
        raise ValueError("partition needs labels [n]")
    n = labels.numel()
    if K < 1 or n >= 1 << 32:
        raise ValueError(f"partition needs K >= 1 and fewer than 2^32 rows, got K = {K}, n = {n}")
    if not labels.is_cuda or K > PARTITION_MAX_K:
        out = cpu.partition(labels, K)
        return out if want_pos else out[:2]
    C = require()
    assert C.PARTITION_MAX_K == PARTITION_MAX_K
    lab = labels.to(torch.int32).contiguous()
    dev = lab.device
    order = torch.empty(n, dtype=torch.int64, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int64, device=dev)
    cells = torch.empty(K * C.partition_blocks(n, K), dtype=torch.int64, device=dev)
    rpos = torch.empty(n, dtype=torch.int64, device=dev) if want_pos else None
    C.partition(lab, K, order, offsets, cells, rpos)
    return (order, offsets, rpos) if want_pos else (order, offsets)


def index_tiles(n: int, K: int) -> int:
    """16-row tiles of an index's row pack: every list padded to whole tiles takes at most
    ``(n + 15 K) // 16`` of them whatever the list sizes (so the allocation needs no host read)."""
    return (int(n) + 15 * int(K)) // 16


class RowIndex:
    """The tensors of one index (all on one device):

    ``n`` the ids handed out so far (the rows of the build and every row added since, whether in a
    list or not; fewer than 2^32), ``pack`` the rows, list after list and each list padded to whole 16-row tiles (fragment-packed
    as :func:`mikmeans.ops.pack_centers` packs centres where ``native``, ``[16 tiles, cols]`` natural
    rows otherwise), ``cn`` their squared norms, ``order`` (int64 [n], tail -1) the row ids list after
    list, ``offsets`` / ``tile_offsets`` (int64 [K + 1]) where each list starts in ``order`` / in tiles."""

    def __init__(self, n, K, D, dtype, native, cols, pack, cn, order, offsets, tile_offsets):
        self.n, self.K, self.D, self.dtype, self.native, self.cols = n, K, D, dtype, native, cols
        self.pack, self.cn, self.order, self.offsets, self.tile_offsets = pack, cn, order, offsets, tile_offsets

    def tensors(self) -> dict:
        return {"row_pack": self.pack, "cn": self.cn, "order": self.order, "offsets": self.offsets,
                "tile_offsets": self.tile_offsets}

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors().values())


def _native_cols(Xp: torch.Tensor) -> int:
    return dpad_for(Xp.shape[1], Xp.dtype) if Xp.is_cuda else 0


def _nearest_lists(labels: torch.Tensor, start: int, blocks, centers, block_rows, like: RowIndex | None = None):
    """``labels[start + i]`` = the list of row i of ``blocks``: :func:`topk`'s first column, -1 where its
    distance is NaN or infinite.  Returns the rows' ``(D, dtype, native cols)``, which must be those of
    the index ``like`` where one is given."""
    shape = None
    for s, Xt, pk in blocks():
        Xp = pad_columns(Xt) if Xt.is_cuda else Xt
        held = like is not None and (like.D, like.dtype, labels.device)
        if held and (Xp.dim() != 2 or (Xp.shape[1], Xp.dtype, Xp.device) != held):
            raise ValueError(f"the index holds rows of {like.D} {like.dtype} features on {labels.device}, got "
                             f"{tuple(Xp.shape)} {Xp.dtype} on {Xp.device}")
        shape = (Xp.shape[1], Xp.dtype, _native_cols(Xp))
        for s2, idx, d2 in topk_blocks(Xp, centers, 1, pack=pk, block_rows=block_rows):
            a = start + s + s2
            labels[a : a + idx.shape[0]] = torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1)
    return shape


def _layout(labels: torch.Tensor, K: int, cols: int, dtype):
    """``(order, offsets, rpos, toff, rpack, cn)`` of the index whose ids have the lists ``labels``:
    the partition, every list's first tile and an empty row pack (zeros, ``PAD_SCORE`` in ``cn``)."""
    n, dev = labels.numel(), labels.device
    order, offsets, rpos = partition(labels, K, want_pos=True)
    sizes = offsets[1:] - offsets[:-1]
    toff = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    toff[1:] = torch.cumsum((sizes + 15) // 16, 0)
    tiles = index_tiles(n, K)
    rpack = torch.zeros(tiles * 16 * cols, dtype=dtype, device=dev)
    cn = torch.full((tiles * 16,), cpu.PAD_SCORE, dtype=torch.float32, device=dev)
    return order, offsets, rpos, toff, rpack, cn


def _pack_rows(blocks, start: int, native: bool, cols: int, labels, rpos, offsets, toff, rpack, cn) -> None:
    """The rows of ``blocks`` (ids from ``start`` on) into the row pack."""
    for s, Xt, _ in blocks():
        if native:
            require().ivf_pack(pad_columns(Xt), start + s, labels, rpos, offsets, toff, rpack, cn, cols)
        else:
            cpu.index_pack(Xt, start + s, labels, rpos, offsets, toff, rpack.view(-1, cols), cn)


def index_build(X, centers: torch.Tensor, *, pack=None, block_rows: int | None = None, blocks=None,
                n: int | None = None) -> RowIndex:
    """Index the rows of ``X`` under ``centers``.  A row's list is :func:`topk`'s first column (the
    exact nearest centre, the lower index on ties); rows whose distance to it is NaN or infinite are
    in no list.  ``blocks`` (with ``n``, instead of ``X``): a callable giving an iterator of
    ``(start, rows, centre pack)`` over the ``n`` rows, walked twice (lists, then the row pack) --
    host rows cross to the device block by block.  ``block_rows``: rows per top-1 pass.  The index
    does not depend on either blocking."""
    if blocks is None:
        n, blocks = X.shape[0], (lambda: [(0, X, pack)])
    n, K = int(n), int(centers.shape[0])
    if n >= 1 << 32:
        raise ValueError(f"an index takes fewer than 2^32 rows, got {n}")
    labels = torch.empty(n, dtype=torch.int32, device=centers.device)
    D, dtype, dpad = _nearest_lists(labels, 0, blocks, centers, block_rows)
    cols = dpad or D
    order, offsets, rpos, toff, rpack, cn = _layout(labels, K, cols, dtype)
    _pack_rows(blocks, 0, bool(dpad), cols, labels, rpos, offsets, toff, rpack, cn)
    return RowIndex(n, K, D, dtype, bool(dpad), cols, rpack, cn, order, offsets, toff)


def _id_lists(index: RowIndex):
    """``(labels int32 [n], rpos int64 [n])`` of an index: every id's list and its position in
    ``order``, -1 for an id in no list -- ``rpos[order[i]] = i`` and the bucket of ``i`` in
    ``offsets`` -- on the index's device, without a host read."""
    n, dev = index.n, index.order.device
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    held = index.order >= 0                                   # (order's tail is -1)
    at = torch.where(held, index.order, n)                    # the tail writes slot n, which is dropped
    rpos = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    rpos[at] = torch.where(held, pos, -1)
    labels = torch.full((n + 1,), -1, dtype=torch.int32, device=dev)
    labels[at] = torch.where(held, torch.bucketize(pos, index.offsets[1:], right=True), -1).to(torch.int32)
    return labels[:n], rpos[:n]


def _update(index: RowIndex, labels: torch.Tensor, rpos_old: torch.Tensor, blocks=None) -> RowIndex:
    """The index whose ids have the lists ``labels`` (int32 [n], the ids of ``index`` first): the
    partition, fresh buffers, the rows of ``index`` that keep a list copied from its pack (they
    keep their list: only -1 may replace a label) and the rows of ``blocks`` -- ``(start, rows,
    centre pack)`` with ``start`` counted from ``index.n`` -- packed behind them."""
    n, K, cols = labels.numel(), index.K, index.cols
    order, offsets, rpos, toff, rpack, cn = _layout(labels, K, cols, index.dtype)
    if index.native:
        require().ivf_repack(index.pack, index.cn, index.offsets, index.tile_offsets, rpos_old, order, offsets, toff,
                             rpack, cn, index.D, cols)
    else:
        cpu.index_repack(index.pack.view(-1, cols), index.cn, index.offsets, index.tile_offsets, rpos_old, labels, rpos,
                         offsets, toff, rpack.view(-1, cols), cn)
    if blocks is not None:
        _pack_rows(blocks, index.n, index.native, cols, labels, rpos, offsets, toff, rpack, cn)
    return RowIndex(n, K, index.D, index.dtype, index.native, cols, rpack, cn, order, offsets, toff)


def index_add(index: RowIndex, X, centers: torch.Tensor, *, pack=None, block_rows: int | None = None, blocks=None,
              n: int | None = None) -> RowIndex:
    """``index`` with the rows of ``X`` added: a new :class:`RowIndex`, equal tensor for tensor to
    :func:`index_build` over the old rows followed by the new ones (where no row was removed).  The
    new rows take the ids ``index.n + i``; a row's list comes from the rule of the build (a row
    whose nearest distance is NaN or infinite takes an id and is in no list), and within a list the
    old rows come first, in their old order, then the new rows ascending.  Only the new rows meet
    the centres and the row pack; the old rows are copied from the old pack into the new one, bits
    as stored (csrc/ivf.hip: the repack).  ``blocks`` / ``n`` / ``block_rows``: as in
    :func:`index_build`, over the new rows alone."""
    if blocks is None:
        n, blocks = X.shape[0], (lambda: [(0, X, pack)])
    n0, n1, K = index.n, int(n), index.K
    if int(centers.shape[0]) != K:
        raise ValueError(f"the index has {K} lists, the centres are {int(centers.shape[0])}")
    if n0 + n1 >= 1 << 32:
        raise ValueError(f"an index takes fewer than 2^32 ids, got {n0} + {n1}")
    dev = index.order.device
    labels = torch.empty(n0 + n1, dtype=torch.int32, device=dev)
    labels[:n0], rpos_old = _id_lists(index)
    _nearest_lists(labels, n0, blocks, centers, block_rows, like=index)
    return _update(index, labels, rpos_old, blocks)


def index_remove(index: RowIndex, ids: torch.Tensor):
    """``index`` without the rows ``ids`` (int64 local row ids, in any order): ``(RowIndex, removed)``,
    ``removed`` an int64 0-d tensor on the index's device, the rows that left a list.  Duplicates,
    ids out of range, ids in no list and ids removed before are ignored.  The rows that stay keep
    their ids and their order, the lists close up and ``n`` stays (an id is never handed out
    twice): the result equals :func:`index_build` over the rows that stay, ``order`` mapped back to
    the old ids.  The rows are copied from the old pack, bits as stored; no host read is made."""
    ids = torch.as_tensor(ids)
    if ids.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"remove takes integer row ids, got {ids.dtype}")
    n, dev = index.n, index.order.device
    ids = ids.reshape(-1).to(device=dev, dtype=torch.int64)
    labels, rpos_old = _id_lists(index)
    named = torch.zeros(n + 1, dtype=torch.bool, device=dev)
    named[torch.where((ids >= 0) & (ids < n), ids, n)] = True   # ids out of range name slot n, which is dropped
    gone = named[:n] & (labels >= 0)
    removed = gone.sum()
    return _update(index, torch.where(gone, -1, labels), rpos_old), removed


def pair_items(index: RowIndex, probes: torch.Tensor, P: int):
    """The work items of a walk over the lists ``probes`` (int [nq, nprobe]) names, ``P`` blocks of 16
    pairs an item (csrc/walk.h): ``(porder, poff, icum, max_items)`` -- the pair ids
    ``q * nprobe + j`` grouped by list, where each list's pairs start, the cumulative item counts
    and the grid bound ``walk_max_items``, which needs no host read.  The only place ``icum`` is
    formed."""
    npairs, per = probes.numel(), 16 * int(P)
    porder, poff = partition(probes.reshape(-1), index.K)
    icum = torch.zeros(index.K + 1, dtype=torch.int64, device=probes.device)
    icum[1:] = torch.cumsum((poff[1:] - poff[:-1] + per - 1) // per, 0)
    return porder, poff, icum, npairs // per + min(index.K, npairs)


def _walk_args(index: RowIndex, Qp: torch.Tensor, probes: torch.Tensor, P: int, *mid) -> tuple:
    """The leading arguments of ``ivf_scan`` / ``ivf_range`` (``mid``: what the op takes after ``qn``)."""
    porder, poff, icum, max_items = pair_items(index, probes, P)
    return (Qp, row_sqnorm(Qp), *mid, index.pack, index.cn, index.offsets, index.tile_offsets, index.order, porder,
            poff, icum, probes.shape[1], index.cols, P, max_items)


def _scan(index: RowIndex, Qp: torch.Tensor, probes: torch.Tensor, m: int) -> torch.Tensor:
    """Sorted keys int64 [nq, m] of one block of queries (native)."""
    C = require()
    nq, nprobe = probes.shape
    P = C.ivf_scan_blocks(dtype_code(Qp.dtype), index.cols, m, nq * nprobe)
    out = torch.empty((nq * nprobe, m), dtype=torch.int64, device=Qp.device)
    C.ivf_scan(*_walk_args(index, Qp, probes, P), out)
    return out.view(nq, nprobe * m).sort(dim=1).values[:, :m]   # unique keys: any sort gives one order


def _check_queries(what: str, index: RowIndex, Q: torch.Tensor, nprobe: int) -> torch.Tensor:
    """The queries of a ``what`` ("search" / "range search") as the index takes them (columns padded
    on the GPU), or a ValueError."""
    if not 1 <= nprobe <= index.K:
        raise ValueError(f"{what} needs 1 <= nprobe <= n_clusters ({index.K}), got nprobe = {nprobe}")
    Qp = pad_columns(Q) if Q.is_cuda else Q
    if Qp.shape[1] != index.D or Qp.dtype != index.dtype or Qp.device != index.pack.device:
        raise ValueError(f"{what} needs queries of {index.D} {index.dtype} features on {index.pack.device}, got "
                         f"{Qp.shape[1]} {Qp.dtype} on {Qp.device}")
    return Qp


def index_search(index: RowIndex, Q: torch.Tensor, centers: torch.Tensor, m: int, nprobe: int, *,
                 pack=None) -> torch.Tensor:
    """The ``m`` nearest indexed rows of every query among the lists of its ``nprobe`` nearest centres
    (:func:`topk`'s indices): int64 keys ``[nq, m]``, ``d2 bits << 32 | row``, ascending -- so equal
    distances go to the lower row -- and ``IVF_EMPTY_KEY`` where the probed lists hold fewer than
    ``m`` rows.  ``d2`` is bitwise ``transform(Q, X.float(), squared=True)``'s value for the pair.
    ``pack``: the centres' pack, as in :func:`topk`."""
    m, nprobe = int(m), int(nprobe)
    if not 1 <= m <= INDEX_MAX_M:
        raise ValueError(f"search needs 1 <= m <= {INDEX_MAX_M}, got m = {m}")
    Qp = _check_queries("search", index, Q, nprobe)
    nq = Qp.shape[0]
    if not index.native:
        return cpu.index_search(index, Qp, centers, m, nprobe)
    keys = torch.empty((nq, m), dtype=torch.int64, device=Qp.device)
    block = max(1, INDEX_SCAN_KEYS // (nprobe * m))
    for s in range(0, nq, block):
        Qb = Qp[s : s + block]
        probes, _ = topk(Qb, centers, nprobe, pack=pack)
        keys[s : s + block] = _scan(index, Qb, probes, m)
    return keys


def _range_block(index: RowIndex, Qp: torch.Tensor, probes: torch.Tensor, r2: torch.Tensor, count_only: bool):
    """``(counts int64 [nq * nprobe], keys int64 [total] or None)`` of one block of queries (native):
    every (query, probe) pair's hits and, unless ``count_only``, their keys in pair-id order (query
    after query, probe after probe) and in list order within a pair.  The fill pass costs one host
    read of the block's total."""
    C = require()
    npairs, dev = probes.numel(), Qp.device
    P = C.ivf_range_blocks(dtype_code(Qp.dtype), index.cols, npairs)
    counts = torch.zeros(npairs, dtype=torch.int64, device=dev)
    args = (*_walk_args(index, Qp, probes, P, r2), counts)
    C.ivf_range(*args)
    if count_only:
        return counts, None
    end = torch.cumsum(counts, 0)
    keys = torch.empty(int(end[-1]), dtype=torch.int64, device=dev)   # (the host read)
    if keys.numel():
        C.ivf_range(*args, end - counts, keys)
    return counts, keys


def index_range(index: RowIndex, Q: torch.Tensor, centers: torch.Tensor, r2, nprobe: int, *, pack=None,
                sort: bool = True, count_only: bool = False, block_queries: int | None = None,
                want_probe: bool = False):
    """Every indexed row within a squared radius of each query, among the lists of the query's
    ``nprobe`` nearest centres (:func:`topk`'s indices): ``(lims int64 [nq + 1], keys int64 [total])``,
    query q's hits ``keys[lims[q]:lims[q + 1]]`` as ``d2 bits << 32 | row`` (:func:`index_decode`).  A
    row is a hit where the kernel's float32 ``d2`` -- bitwise ``transform(Q, X.float(),
    squared=True)``'s value for the pair, as in :func:`index_search` -- has ``d2 <= r2[q]``; ``r2``:
    one finite non-negative float32 per query (or one for all).  A NaN or infinite ``d2`` is no hit.

    ``sort``: a query's keys ascending (nearest first, equal distances by the lower row: two stable
    sorts over a block's keys, by key and then by query); otherwise probe after probe, nearest
    centre first, and in list order (ascending row) within a probe, as the kernel writes them.
    ``count_only``: the count pass alone, ``counts int64 [nq]`` (``lims[1:] - lims[:-1]``; nothing is
    allocated per hit and no host read is made).  ``want_probe``: also every hit's probe rank (int64
    [total]).  Queries go through in blocks of ``block_queries`` (default ``INDEX_SCAN_KEYS //
    nprobe``) so that a block's pair arrays stay bounded; each block's fill pass costs one host read
    of its total, which a variable-length result cannot avoid.  A long list is not split over
    waves.  The result does not depend on the blocking and is bitwise the same from run to run."""
    nprobe = int(nprobe)
    if Q.dim() != 2:
        raise ValueError(f"range search needs queries [nq, D], got shape {tuple(Q.shape)}")
    Qp = _check_queries("range search", index, Q, nprobe)
    nq, dev = Qp.shape[0], Qp.device
    r2 = torch.as_tensor(r2, dtype=torch.float32, device=dev)
    if r2.dim() > 1 or (r2.dim() == 1 and r2.shape[0] != nq):
        raise ValueError(f"range search needs one squared radius, or one per query ({nq}), got shape {tuple(r2.shape)}")
    r2 = r2.expand(nq).contiguous()
    if nq and not bool((torch.isfinite(r2) & (r2 >= 0)).all()):
        raise ValueError("range search needs finite non-negative squared radii")
    if not index.native:
        return cpu.index_range(index, Qp, centers, r2, nprobe, sort=sort, count_only=count_only, want_probe=want_probe)
    block = max(1, int(block_queries) if block_queries else INDEX_SCAN_KEYS // nprobe)
    cq, keys, ranks = [], [], []
    for s in range(0, nq, block):
        Qb = Qp[s : s + block]
        nb = Qb.shape[0]
        probes, _ = topk(Qb, centers, nprobe, pack=pack)
        counts, kb = _range_block(index, Qb, probes, r2[s : s + block], count_only)
        cq.append(counts.view(nb, nprobe).sum(1))
        if count_only:
            continue
        pr = None
        if want_probe:
            pr = torch.repeat_interleave(torch.arange(nb * nprobe, device=dev), counts, output_size=kb.numel()) % nprobe
        if sort:
            qid = torch.repeat_interleave(torch.arange(nb, device=dev), cq[-1], output_size=kb.numel())
            kb, o1 = kb.sort()                                    # unique keys: any sort gives one order
            o2 = qid[o1].sort(stable=True).indices
            kb = kb[o2]
            pr = pr[o1][o2] if want_probe else None
        keys.append(kb)
        ranks.append(pr)
    cq = torch.cat(cq) if cq else torch.zeros(0, dtype=torch.int64, device=dev)
    if count_only:
        return cq
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(cq, 0)
    keys = torch.cat(keys) if keys else torch.zeros(0, dtype=torch.int64, device=dev)
    if want_probe:
        return lims, keys, (torch.cat(ranks) if ranks else torch.zeros(0, dtype=torch.int64, device=dev))
    return lims, keys


def deep_block_queries(m: int, nprobe: int) -> int:
    """Queries per block of a deep search: the histogram (1 KiB a query), the pair arrays (porder,
    probes, counts and base: 28 B a pair) and ``INDEX_DEEP_OVERSHOOT * m`` keys a query within
    ``INDEX_SCAN_KEYS`` keys' worth of bytes."""
    per = 4 * QUANTILE_BINS + 28 * int(nprobe) + 8 * INDEX_DEEP_OVERSHOOT * int(m)
    return max(1, 8 * INDEX_SCAN_KEYS // per)


def index_hist(index: RowIndex, Q: torch.Tensor, probes: torch.Tensor, pass_: int, prefix: torch.Tensor | None = None,
               *, table: torch.Tensor | None = None, P: int | None = None, walk: tuple | None = None) -> torch.Tensor:
    """One radix-select pass's histogram of a deep search (csrc/deep.hip): every row of the lists
    ``probes`` (int [nq, nprobe]) names for a query adds one to the query's 256 bins by a digit of
    its ``d2`` bits -- ``bits >> 24`` in pass 0; ``(bits >> s) & 255``, ``s = 24 - 8 * pass``, where
    ``bits >> (s + 8)`` is ``prefix[q]``'s (int32 [nq]) in passes 1..3.  Rows at an infinite or NaN
    distance count too.  Native: u32 counts as int32 ``[nq, 256]``, added into ``table`` where one is
    given (else a zeroed one); ``P``: pair blocks a wave (``ivf_hist_blocks`` or 1: the same table);
    ``walk``: the walk's arguments where the caller holds them (``_walk_args`` at ``P``).  A CPU index
    runs :func:`mikmeans.ops.cpu.index_hist` (int64)."""
    Qp = _check_queries("search", index, Q, probes.shape[1])
    if not index.native:
        bits, member, _ = cpu.index_pair_bits(index, Qp, probes)
        return cpu.index_hist(bits, member, prefix, pass_)
    C = require()
    if walk is None:
        P = int(P) if P else C.ivf_hist_blocks(dtype_code(Qp.dtype), index.cols, probes.numel())
        walk = _walk_args(index, Qp, probes, P)
    if table is None:
        table = torch.zeros((Qp.shape[0], QUANTILE_BINS), dtype=torch.int32, device=Qp.device)
    C.ivf_hist(*walk, table, prefix if int(pass_) else None, int(pass_))
    return table


def index_select(table: torch.Tensor, prefix: torch.Tensor, rank: torch.Tensor, hits: torch.Tensor,
                 cand: torch.Tensor, m: int, pass_: int) -> None:
    """One select step of a deep search, in place (csrc/deep.hip; :func:`mikmeans.ops.cpu.index_select`
    has the rule): ``prefix`` int32, ``rank`` / ``hits`` / ``cand`` int64, all ``[nq]``."""
    if table.is_cuda:
        require().ivf_select(table, prefix, rank, hits, cand, int(m), int(pass_))
        return
    for dst, src in zip((prefix, rank, hits, cand), cpu.index_select(table, prefix, rank, cand, m, pass_)):
        dst.copy_(src)


def _deep_radius(index: RowIndex, Qp: torch.Tensor, probes: torch.Tensor, m: int, passes: int | None):
    """``(r2 float32 [nq], passes run)`` of one block of queries (native): the radix select's prefix
    after the last pass run with every lower bit set, as a float32 bit pattern -- at least every
    query's ``min(m, candidates)``-th smallest ``d2``, and exactly it after four passes.  It may be
    an inf or NaN pattern: it is formed by integer ops and only ever compared as bits."""
    C = require()
    nq, dev = Qp.shape[0], Qp.device
    P = C.ivf_hist_blocks(dtype_code(Qp.dtype), index.cols, probes.numel())
    walk = _walk_args(index, Qp, probes, P)
    table = torch.empty((nq, QUANTILE_BINS), dtype=torch.int32, device=dev)
    prefix = torch.zeros(nq, dtype=torch.int32, device=dev)
    rank, hits, cand = (torch.zeros(nq, dtype=torch.int64, device=dev) for _ in range(3))
    for p in range(cpu.QUANTILE_PASSES):
        table.zero_()
        index_hist(index, Qp, probes, p, prefix, table=table, walk=walk)
        index_select(table, prefix, rank, hits, cand, m, p)
        if p + 1 == (passes or cpu.QUANTILE_PASSES):
            break
        # (the one host read of the pass: one more walk against the fill and sort volume)
        if passes is None and bool(hits.sum() <= INDEX_DEEP_OVERSHOOT * cand.clamp(max=m).sum()):
            break
    return (prefix | ((1 << (24 - 8 * p)) - 1)).view(torch.float32), p + 1


def _deep_collect(index: RowIndex, Qp: torch.Tensor, probes: torch.Tensor, r2: torch.Tensor, m: int) -> torch.Tensor:
    """Sorted keys int64 [nq, m] of one block of queries (native) from a radius that lets at least
    every query's ``min(m, candidates)`` nearest rows through: the range passes' count, cumulative
    sum and fill, the sort by unique keys and every query's first ``m``."""
    nq, dev = Qp.shape[0], Qp.device
    counts, kb = _range_block(index, Qp, probes, r2, False)
    cq = counts.view(nq, -1).sum(1)
    qid = torch.repeat_interleave(torch.arange(nq, device=dev), cq, output_size=kb.numel())
    kb, o1 = kb.sort()                                        # unique keys: any sort gives one order
    o2 = qid[o1].sort(stable=True).indices
    kb, qid = kb[o2], qid[o1][o2]
    pos = torch.arange(kb.numel(), device=dev) - (torch.cumsum(cq, 0) - cq)[qid]
    keep = pos < m
    keys = torch.full((nq, m), IVF_EMPTY_KEY, dtype=torch.int64, device=dev)
    keys[qid[keep], pos[keep]] = kb[keep]
    return keys


def index_search_deep(index: RowIndex, Q: torch.Tensor, centers: torch.Tensor, m: int, nprobe: int, *, pack=None,
                      passes: int | None = None, block_queries: int | None = None) -> torch.Tensor:
    """:func:`index_search` past the scan kernel's list: the ``m`` nearest indexed rows of every query
    among the lists of its ``nprobe`` nearest centres for ``1 <= m <= INDEX_DEEP_MAX_M`` -- the same
    int64 keys ``[nq, m]``, ``d2 bits << 32 | row`` ascending, ``IVF_EMPTY_KEY`` where the lists hold
    fewer rows, and for ``m <= INDEX_MAX_M`` :func:`index_search`'s bit for bit.

    No candidate list is kept.  A most-significant-digit radix select over the ``d2`` bits
    (csrc/deep.hip: a histogram pass over the walk and a select per 8-bit digit, csrc/quantiles.hip's
    method) finds a radius that is at least every query's m-th smallest ``d2`` -- after four passes
    exactly it -- and the range passes (csrc/range.hip) collect the rows under it; each query keeps
    the first ``m`` of its sorted keys.  The loop stops after any pass where the radius lets through
    at most ``INDEX_DEEP_OVERSHOOT`` times the rows wanted over the block (one scalar host read a
    pass): one more walk is traded against fill and sort volume, and the result does not depend on
    it.  ``passes`` = 1..4 forces the pass count.  Rows at the m-th distance are all under the exact
    radius: ties there make the rows collected exceed ``m`` by the number of tied rows (the lower row
    ids are kept), which is inherent to the method.  Queries go through in blocks
    (:func:`deep_block_queries`, or ``block_queries``); the result does not depend on the blocking
    and is bitwise the same from run to run.  A CPU index runs the mirror of :func:`index_search`."""
    m, nprobe = int(m), int(nprobe)
    if not 1 <= m <= INDEX_DEEP_MAX_M:
        raise ValueError(f"search_deep needs 1 <= m <= {INDEX_DEEP_MAX_M}, got m = {m}")
    if passes is not None and not 1 <= int(passes) <= cpu.QUANTILE_PASSES:
        raise ValueError(f"search_deep needs passes in 1..{cpu.QUANTILE_PASSES} (or None), got {passes}")
    if Q.dim() != 2:
        raise ValueError(f"search_deep needs queries [nq, D], got shape {tuple(Q.shape)}")
    Qp = _check_queries("search_deep", index, Q, nprobe)
    nq = Qp.shape[0]
    if not index.native:
        return cpu.index_search(index, Qp, centers, m, nprobe)
    keys = torch.empty((nq, m), dtype=torch.int64, device=Qp.device)
    block = max(1, int(block_queries)) if block_queries else deep_block_queries(m, nprobe)
    for s in range(0, nq, block):
        Qb = Qp[s : s + block]
        probes, _ = topk(Qb, centers, nprobe, pack=pack)
        r2, _ = _deep_radius(index, Qb, probes, m, None if passes is None else int(passes))
        keys[s : s + block] = _deep_collect(index, Qb, probes, r2, m)
    return keys


def index_decode(keys: torch.Tensor, *, row_start: int = 0):
    """``(rows int64, d2 float32)`` of search keys: each slot's row (plus ``row_start``) and squared
    distance, -1 and NaN for the empty slots."""
    empty = keys == IVF_EMPTY_KEY
    rows = torch.where(empty, -1, (keys & 0xFFFFFFFF) + int(row_start))
    d2 = torch.where(empty, 0, keys >> 32).to(torch.int32).view(torch.float32)
    return rows, torch.where(empty, float("nan"), d2)
