"""The fitted clusters as a product-quantised index (IVF-PQ): one byte per sub-vector instead of the row.

A row in list ``l`` is kept as the ``M`` codes of its residual ``x - centers[l]``: the residual's
``F`` features are cut into ``M`` sub-vectors of ``dsub = F // M`` and each is replaced by the nearest
of 256 codewords of its sub-space.  A query meets a list through a table of its own residual's
squared distances to every codeword, and a row's asymmetric distance ("ADC") is the sum of ``M``
table entries.  Everything is defined bit for bit (docs/PQ_INDEX.md):

* :func:`pq_train`    the codebooks: this library's own :class:`mikmeans.KMeans` with 256 centres in
  every sub-space
* :func:`pq_encode`   ``code[i, j]`` = :func:`mikmeans.ops.topk`'s nearest codeword (m = 1) of sub-vector j
* :func:`pq_lut`      ``lut[p, j, :]`` = :func:`mikmeans.ops.transform`'s squared distances of sub-vector j
* :func:`pq_build`    the lists of :func:`mikmeans.ops.index_build`, the training sample and the codes,
  list after list: a :class:`PQRowIndex`
* :func:`pq_search`   the ``nprobe`` nearest centres of every query, the tables of its residuals and
  the scan of csrc/pq.hip: sorted ``(ADC bits << 32 | row)`` keys, decoded by
  :func:`mikmeans.ops.index_decode`
* :func:`pq_shortlist` / :func:`rerank` / :func:`pq_refine`   the refined search: the scan picks a
  shortlist of every probed list and csrc/rerank.hip ranks it by exact distances to the rows

GPU tensors run the native kernels; CPU tensors run the mirrors of :mod:`mikmeans.ops.cpu` with the
same tensors and the same order of adds.
"""
from __future__ import annotations

import torch

from . import cpu, pack_centers, pad_columns, topk, transform
from .index import INDEX_MAX_M, _nearest_lists, partition
from .native import dpad_for, require

__all__ = ["PQ_SUBVECTORS", "PQ_KSUB", "PQ_SCAN_BYTES", "PQ_ENCODE_ROWS", "PQRowIndex", "pq_check", "pq_train",
           "pq_encode", "pq_lut", "pq_build", "pq_search", "pq_block_queries", "pq_reconstruct", "pq_shortlist",
           "pq_shortlist_groups", "pq_refine", "pq_refine_block_queries", "rerank"]

PQ_SUBVECTORS = cpu.PQ_SUBVECTORS    # csrc/pqplan.h pq_subvectors_ok
PQ_KSUB = cpu.PQ_KSUB                # codewords of a sub-space: a code is one byte
PQ_SCAN_BYTES = 1 << 30              # tables, residuals and keys of one block of queries
PQ_ENCODE_ROWS = 1 << 18             # rows per encoding pass (their float32 residuals: 512 B a row at F = 128)


def pq_check(F: int, M: int) -> int:
    """``dsub`` of ``F`` features in ``M`` sub-vectors, or a ValueError that names what is allowed."""
    F, M = int(F), int(M)
    if M not in PQ_SUBVECTORS or F % M != 0:
        raise ValueError(f"a PQ index takes n_subvectors in {PQ_SUBVECTORS} that divide the {F} features, got {M}")
    return F // M


def _codebook_packs(codebooks: torch.Tensor, dtype):
    """The codebooks packed for the MFMA kernels, one pack a sub-space (None where the kernels do not run)."""
    if not codebooks.is_cuda:
        return None
    cols = pad_columns(torch.empty((0, codebooks.shape[2]), dtype=dtype)).shape[1]
    if dpad_for(cols, dtype) == 0:
        return None
    return [pack_centers(cb, cols, dtype, codebooks.device) for cb in codebooks]


def pq_train(R: torch.Tensor, M: int, *, max_iter: int = 25, seed: int = 0) -> torch.Tensor:
    """Codebooks float32 ``[M, 256, dsub]`` of the residuals ``R`` ``[n, F]`` (bfloat16 or float32): in
    sub-space j -- columns ``[j dsub, (j + 1) dsub)`` -- :class:`mikmeans.KMeans` with 256 centres,
    ``R``'s dtype, ``max_iter`` and the seed ``(seed * 1000003 + j) mod 2^31`` fits the contiguous
    slice.  The same inputs and seed give the same codebooks bit for bit."""
    from ..api import KMeans

    n, F = R.shape
    dsub = pq_check(F, M)
    if n < PQ_KSUB:
        raise ValueError(f"PQ training needs at least {PQ_KSUB} rows, got {n}")
    out = torch.empty((int(M), PQ_KSUB, dsub), dtype=torch.float32, device=R.device)
    for j in range(int(M)):
        km = KMeans(PQ_KSUB, dtype=R.dtype, max_iter=int(max_iter), device=R.device,
                    seed=(int(seed) * 1000003 + j) & 0x7FFFFFFF)
        km.fit(R[:, j * dsub : (j + 1) * dsub].contiguous())
        out[j] = km.cluster_centers_.to(torch.float32)
    return out


def pq_encode(R: torch.Tensor, codebooks: torch.Tensor, *, packs=None) -> torch.Tensor:
    """Codes uint8 ``[n, M]``: ``code[i, j] = topk(R[:, slice_j], codebooks[j], 1)[0][i, 0]``, the exact
    nearest codeword and the lower index on ties.  ``packs``: the codebooks' packs where the caller holds them."""
    M, _, dsub = codebooks.shape
    if R.shape[1] != M * dsub:
        raise ValueError(f"the codebooks take rows of {M * dsub} features, got {R.shape[1]}")
    if not R.is_cuda:
        return cpu.pq_encode(R, codebooks)
    codes = torch.empty((R.shape[0], M), dtype=torch.uint8, device=R.device)
    for j in range(M):
        idx, _ = topk(R[:, j * dsub : (j + 1) * dsub], codebooks[j], 1, pack=packs[j] if packs else None)
        codes[:, j] = idx[:, 0].to(torch.uint8)
    return codes


def pq_lut(RQ: torch.Tensor, codebooks: torch.Tensor, *, packs=None) -> torch.Tensor:
    """Tables float32 ``[npairs, M, 256]``: ``lut[p, j, :] = transform(RQ[:, slice_j], codebooks[j],
    squared=True)[p]``; every entry is ``>= +0``, or NaN / inf for a non-finite residual."""
    M, _, dsub = codebooks.shape
    if RQ.shape[1] != M * dsub:
        raise ValueError(f"the codebooks take rows of {M * dsub} features, got {RQ.shape[1]}")
    if not RQ.is_cuda:
        return cpu.pq_lut(RQ, codebooks)
    lut = torch.empty((RQ.shape[0], M, PQ_KSUB), dtype=torch.float32, device=RQ.device)
    for j in range(M):
        lut[:, j, :] = transform(RQ[:, j * dsub : (j + 1) * dsub], codebooks[j], squared=True,
                                 pack=packs[j] if packs else None)
    return lut


class PQRowIndex:
    """The tensors of one product-quantised index (all on one device):

    ``n`` the rows given (fewer than 2^32), ``K`` lists, ``D`` the rows' stored columns (padded to 16
    bytes on the GPU), ``M`` sub-vectors, ``dtype`` the rows' dtype; ``codes`` uint8 ``[n, M]`` the codes
    of the rows of ``order`` position after position -- list ``l`` is ``codes[offsets[l]:offsets[l + 1]]``,
    no per-list padding, the unused tail zero -- ``order`` (int64 [n], tail -1), ``offsets`` (int64
    [K + 1]) and ``codebooks`` float32 ``[M, 256, dsub]``."""

    def __init__(self, n, K, D, M, dtype, codes, order, offsets, codebooks):
        self.n, self.K, self.D, self.M, self.dtype = int(n), int(K), int(D), int(M), dtype
        self.codes, self.order, self.offsets, self.codebooks = codes, order, offsets, codebooks
        self._packs = None

    @property
    def F(self) -> int:
        return self.M * int(self.codebooks.shape[2])

    def tensors(self) -> dict:
        return {"codes": self.codes, "order": self.order, "offsets": self.offsets, "codebooks": self.codebooks}

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors().values())

    def packs(self):
        """The codebooks' packs, made once (they are not part of the index: 256 rows a sub-space)."""
        if self._packs is None:
            self._packs = _codebook_packs(self.codebooks, self.dtype) or ()
        return self._packs or None


def _residuals(Xt: torch.Tensor, lists: torch.Tensor, centers: torch.Tensor, dtype) -> torch.Tensor:
    """``(x.float() - centers[list]).to(dtype)`` over the centres' features, formed in float32."""
    F = centers.shape[1]
    return (Xt[:, :F].to(torch.float32) - centers[lists.to(torch.int64)]).to(dtype)


def _sample_positions(n_indexed: int, train_rows: int, seed: int) -> torch.Tensor:
    """``t = min(train_rows, n_indexed)`` positions of ``order`` without replacement, ascending: one
    from each of ``t`` runs of ``n_indexed // t`` positions, drawn by a CPU generator seeded from
    ``seed`` (so the sample does not depend on the device)."""
    t = min(int(train_rows), int(n_indexed))
    g = torch.Generator().manual_seed(int(seed))
    stride = max(1, n_indexed // max(t, 1))
    return torch.arange(t, dtype=torch.int64) * stride + torch.randint(0, stride, (t,), generator=g, dtype=torch.int64)


def pq_build(X, centers: torch.Tensor, M: int, *, codebooks: torch.Tensor | None = None, train_rows: int = 65536,
             max_iter: int = 25, seed: int = 0, pack=None, block_rows: int | None = None, blocks=None,
             n: int | None = None) -> PQRowIndex:
    """Index the rows of ``X`` under ``centers`` as ``M`` one-byte codes a row.  The lists are
    :func:`mikmeans.ops.index_build`'s (the exact nearest centre, the lower index on ties; rows whose
    distance to it is NaN or infinite take an id and are in no list).  Without ``codebooks`` they are
    trained (:func:`pq_train`) on the residuals of ``min(train_rows, n_indexed)`` listed rows, one
    from each of as many equal runs of ``order``, drawn by a CPU generator seeded from ``seed``; that
    costs the build's one host read (the number of listed rows), with ``codebooks`` it makes none.
    ``blocks`` / ``n`` / ``block_rows``: as in :func:`mikmeans.ops.index_build` (the rows are walked
    once for the lists, once for the sample and once for the codes; the residuals are encoded in
    passes of at most ``PQ_ENCODE_ROWS`` rows).  The index does not depend on the blocking."""
    if blocks is None:
        n, blocks = X.shape[0], (lambda: [(0, X, pack)])
    n, K, F = int(n), int(centers.shape[0]), int(centers.shape[1])
    dsub = pq_check(F, M)
    M = int(M)
    if n >= 1 << 32:
        raise ValueError(f"an index takes fewer than 2^32 rows, got {n}")
    dev = centers.device
    if codebooks is not None:
        if tuple(codebooks.shape) != (M, PQ_KSUB, dsub):
            raise ValueError(f"codebooks must be [{M}, {PQ_KSUB}, {dsub}], got {tuple(codebooks.shape)}")
        codebooks = codebooks.to(device=dev, dtype=torch.float32).contiguous()
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    D, dtype, _ = _nearest_lists(labels, 0, blocks, centers, block_rows)
    order, offsets, rpos = partition(labels, K, want_pos=True)
    cen = centers.to(torch.float32)
    if codebooks is None:
        n_indexed = int(offsets[K])                                   # (the host read)
        if n_indexed < PQ_KSUB:
            raise ValueError(f"PQ training needs at least {PQ_KSUB} indexed rows, got {n_indexed}")
        ids = order[_sample_positions(n_indexed, train_rows, seed).to(dev)]
        R = torch.zeros((ids.numel(), F), dtype=dtype, device=dev)
        for s, Xt, _ in blocks():
            nb = Xt.shape[0]
            if nb == 0:
                continue
            here = (ids >= s) & (ids < s + nb)
            at = (ids - s).clamp(0, nb - 1)
            R = torch.where(here[:, None], _residuals(Xt[at], labels[ids], cen, dtype), R)
        codebooks = pq_train(R, M, max_iter=max_iter, seed=seed)
        del R
    packs = _codebook_packs(codebooks, dtype)
    codes = torch.zeros((n + 1, M), dtype=torch.uint8, device=dev)    # (slot n: the rows in no list, dropped)
    step = max(1, min(int(block_rows) if block_rows else PQ_ENCODE_ROWS, PQ_ENCODE_ROWS))
    for s, Xt, _ in blocks():
        for a in range(0, Xt.shape[0], step):
            Xb = Xt[a : a + step]
            lab = labels[s + a : s + a + Xb.shape[0]]
            pos = rpos[s + a : s + a + Xb.shape[0]]
            R = _residuals(Xb, lab.clamp(min=0), cen, dtype)
            codes[torch.where(pos >= 0, pos, n)] = pq_encode(R, codebooks, packs=packs)
    codes[n].zero_()
    index = PQRowIndex(n, K, D, M, dtype, codes[:n], order, offsets, codebooks)
    index._packs = packs or ()
    return index


def pq_block_queries(M: int, m: int, nprobe: int, F: int, splits: int = 8) -> int:
    """Queries per block of a search: a pair's table (``M`` KiB), its residual (float32 and the rows'
    dtype: at most 8 B a feature) and its keys (``splits * m``, with the sort's copy) within ``PQ_SCAN_BYTES``."""
    per = int(nprobe) * (int(M) * PQ_KSUB * 4 + 8 * int(F) + 16 * int(splits) * int(m))
    return max(1, PQ_SCAN_BYTES // per)


def _search_queries(index: PQRowIndex, Q: torch.Tensor, nprobe: int) -> torch.Tensor:
    """The queries as the kernels take them (padded columns on the GPU), or the ValueError of a search."""
    if not 1 <= nprobe <= index.K:
        raise ValueError(f"search needs 1 <= nprobe <= n_clusters ({index.K}), got nprobe = {nprobe}")
    if Q.dim() != 2:
        raise ValueError(f"search needs queries [nq, D], got shape {tuple(Q.shape)}")
    Qp = pad_columns(Q) if Q.is_cuda else Q
    dev = index.codes.device
    if Qp.shape[1] != index.D or Qp.dtype != index.dtype or Qp.device != dev:
        raise ValueError(f"search needs queries of {index.D} {index.dtype} features on {dev}, got "
                         f"{Qp.shape[1]} {Qp.dtype} on {Qp.device}")
    return Qp


def _block_tables(index: PQRowIndex, Qb: torch.Tensor, centers: torch.Tensor, cen: torch.Tensor, nprobe: int, pack):
    """What a block of queries brings to the scan: ``(probes int32 [nb, nprobe], tables float32
    [nb * nprobe, M, 256])`` -- :func:`mikmeans.ops.topk`'s nearest centres and the :func:`pq_lut` of
    every query's residual against each of them.  ``cen``: the centres in float32."""
    nb, F = Qb.shape[0], index.F
    probes, _ = topk(Qb, centers, nprobe, pack=pack)
    RQ = (Qb[:, None, :F].to(torch.float32) - cen[probes.to(torch.int64)]).to(index.dtype).view(nb * nprobe, F)
    return probes, pq_lut(RQ, index.codebooks, packs=index.packs())


def pq_search(index: PQRowIndex, Q: torch.Tensor, centers: torch.Tensor, m: int, nprobe: int, *, pack=None,
              splits: int | None = None, block_queries: int | None = None) -> torch.Tensor:
    """The ``m`` indexed rows of least asymmetric distance to every query among the lists of its
    ``nprobe`` nearest centres (:func:`mikmeans.ops.topk`'s indices): int64 keys ``[nq, m]``, ``ADC bits
    << 32 | row``, ascending -- so equal distances go to the lower row -- and ``IVF_EMPTY_KEY`` where
    the probed lists hold fewer than ``m`` rows.  The ADC of pair ``p = (query, probe)`` and a row with
    codes ``c`` is ``lut[p, 0, c[0]] + lut[p, 1, c[1]] + ...``, float32 adds in that order, ``lut`` the
    :func:`pq_lut` of the query's residual against the probed centre.  ``splits`` (1..8, default
    ``pq_scan_splits`` of the block's pairs): workgroups that share a pair (csrc/pq.hip).  Queries go
    through in blocks (:func:`pq_block_queries`, or ``block_queries``).  The result depends on neither
    and is bitwise the same from run to run."""
    m, nprobe = int(m), int(nprobe)
    if not 1 <= m <= INDEX_MAX_M:
        raise ValueError(f"search needs 1 <= m <= {INDEX_MAX_M}, got m = {m}")
    Qp = _search_queries(index, Q, nprobe)
    dev = index.codes.device
    native = index.codes.is_cuda
    if splits is not None and not 1 <= int(splits) <= cpu.PQ_MAX_SPLITS:
        raise ValueError(f"search needs 1 <= splits <= {cpu.PQ_MAX_SPLITS}, got {splits}")
    nq, F = Qp.shape[0], index.F
    cen = centers.to(torch.float32)
    keys = torch.empty((nq, m), dtype=torch.int64, device=dev)
    block = max(1, int(block_queries)) if block_queries else pq_block_queries(index.M, m, nprobe, F)
    for s in range(0, nq, block):
        Qb = Qp[s : s + block]
        nb = Qb.shape[0]
        probes, lut = _block_tables(index, Qb, centers, cen, nprobe, pack)
        if not native:
            keys[s : s + block] = cpu.pq_scan(index, lut, probes, m)
            continue
        C = require()
        sp = int(splits) if splits is not None else C.pq_scan_splits(nb * nprobe)
        out = torch.empty((nb * nprobe, sp, m), dtype=torch.int64, device=dev)
        C.pq_scan(index.codes, index.order, index.offsets, lut, probes.reshape(-1).contiguous(), sp, out)
        keys[s : s + block] = out.view(nb, nprobe * sp * m).sort(dim=1).values[:, :m]   # unique keys: one order
    return keys


def pq_shortlist_groups(shortlist: int) -> tuple[int, int]:
    """``(G, s)`` of a shortlist of ``S`` rows a probed list: one group of ``S <= 32`` rows, or ``S // 32``
    groups of 32 for ``S`` in 64, 96, ..., 256; a ValueError that names what is allowed otherwise."""
    S = int(shortlist)
    if 1 <= S <= INDEX_MAX_M:
        return 1, S
    if S % INDEX_MAX_M == 0 and 2 <= S // INDEX_MAX_M <= cpu.PQ_MAX_SPLITS:
        return S // INDEX_MAX_M, INDEX_MAX_M
    raise ValueError(f"a shortlist takes 1 <= shortlist <= {INDEX_MAX_M} rows a probed list or one of "
                     f"{', '.join(str(INDEX_MAX_M * g) for g in range(2, cpu.PQ_MAX_SPLITS + 1))}, got {shortlist}")


def pq_refine_block_queries(M: int, nprobe: int, F: int, shortlist: int, *, host_rows: bool = False,
                            esize: int = 4) -> int:
    """Queries per block of a refined search: :func:`pq_block_queries`'s terms at ``splits = G, m = s``,
    a query's ``R = nprobe * shortlist`` candidate ids, its ``R`` re-rank keys with the sort's two copies
    and, for rows kept on the host, the staged rows (at most ``R`` of ``F`` features of ``esize`` bytes)
    and their remapped ids, within ``PQ_SCAN_BYTES``."""
    R = int(nprobe) * int(shortlist)
    per = int(nprobe) * (int(M) * PQ_KSUB * 4 + 8 * int(F) + 16 * int(shortlist)) + 32 * R
    if host_rows:
        per += R * (int(F) * int(esize) + 8)
    return max(1, PQ_SCAN_BYTES // per)


def _shortlist_blocks(index: PQRowIndex, Qp: torch.Tensor, centers: torch.Tensor, G: int, s: int, nprobe: int, pack,
                      block: int):
    """``(first query, candidate ids int64 [nb, nprobe * G * s])`` of every block of the checked queries ``Qp``."""
    cen = centers.to(torch.float32)
    dev = index.codes.device
    for s0 in range(0, Qp.shape[0], block):
        Qb = Qp[s0 : s0 + block]
        nb = Qb.shape[0]
        probes, lut = _block_tables(index, Qb, centers, cen, nprobe, pack)
        if index.codes.is_cuda:
            keys = torch.empty((nb * nprobe, G, s), dtype=torch.int64, device=dev)
            require().pq_scan(index.codes, index.order, index.offsets, lut, probes.reshape(-1).contiguous(), G, keys)
        else:
            keys = cpu.pq_shortlist(index, lut, probes, G, s)
        keys = keys.view(nb, nprobe * G * s)
        yield s0, torch.where(keys == cpu.IVF_EMPTY_KEY, -1, keys & 0xFFFFFFFF)


def pq_shortlist(index: PQRowIndex, Q: torch.Tensor, centers: torch.Tensor, shortlist: int, nprobe: int, *,
                 pack=None, block_queries: int | None = None) -> torch.Tensor:
    """The rows the codes pick for a re-rank: int64 ``[nq, nprobe * S]`` row ids, ``S = shortlist`` a
    probed list, -1 for the empty slots.  ``1 <= S <= 32`` is one group of ``s = S`` rows; ``S`` in 64,
    96, ..., 256 is ``G = S // 32`` groups of ``s = 32``.  Position ``p`` of a list (in ``order``) is in
    group ``(p // 256) mod G``, and a group keeps its ``s`` rows of least ``(ADC bits, row id)``, the ADC
    of :func:`pq_search`.  The slots run probe after probe (the nearest centre first), group after
    group, ascending key within a group.  On the GPU: the scan of csrc/pq.hip with ``splits = G, m = s``,
    whose split ``g`` takes exactly group ``g``.  The result does not depend on the blocking."""
    G, s = pq_shortlist_groups(shortlist)
    nprobe = int(nprobe)
    Qp = _search_queries(index, Q, nprobe)
    block = (max(1, int(block_queries)) if block_queries
             else pq_refine_block_queries(index.M, nprobe, index.F, G * s))
    out = torch.empty((Qp.shape[0], nprobe * G * s), dtype=torch.int64, device=index.codes.device)
    for s0, cand in _shortlist_blocks(index, Qp, centers, G, s, nprobe, pack, block):
        out[s0 : s0 + cand.shape[0]] = cand
    return out


def rerank(Q: torch.Tensor, X: torch.Tensor, cand: torch.Tensor, m: int) -> torch.Tensor:
    """The ``m`` candidates of least exact squared distance to every query: int64 keys ``[nq, m]``,
    ``d2 bits << 32 | row id``, ascending -- equal distances go to the lower row -- and
    ``IVF_EMPTY_KEY`` behind them; :func:`mikmeans.ops.index_decode` decodes them.  ``Q`` ``[nq, F]`` and
    ``X`` ``[n, F]`` (fewer than 2^32 rows) share a dtype (bfloat16 or float32) and a device; ``X`` may be
    a slice with a longer row stride.  ``cand`` int64 ``[nq, R]``: an id outside ``[0, n)`` is an empty
    slot, an id given twice gives its key twice.  ``d2`` is defined bit for bit (docs/PQ_INDEX.md):
    sixteen accumulators over 16-byte pieces, subtract, multiply and add rounded one by one, NaN as one
    pattern.  On the GPU csrc/rerank.hip writes one key per candidate and ``sort`` keeps the ``m``
    smallest; CPU tensors run :func:`mikmeans.ops.cpu.rerank`."""
    m = int(m)
    if m < 1:
        raise ValueError(f"rerank needs m >= 1, got m = {m}")
    if Q.dim() != 2 or X.dim() != 2 or Q.shape[1] != X.shape[1] or Q.shape[1] < 1:
        raise ValueError(f"rerank takes Q [nq, F] and X [n, F], got {tuple(Q.shape)} and {tuple(X.shape)}")
    if Q.dtype != X.dtype or Q.dtype not in (torch.bfloat16, torch.float32) or Q.device != X.device:
        raise ValueError(f"rerank takes bfloat16 or float32 queries and rows of one dtype on one device, got "
                         f"{Q.dtype} on {Q.device} and {X.dtype} on {X.device}")
    if X.shape[0] >= 1 << 32:
        raise ValueError(f"rerank takes fewer than 2^32 rows, got {X.shape[0]}")
    if cand.dim() != 2 or cand.shape[0] != Q.shape[0] or cand.shape[1] < 1 or cand.dtype != torch.int64:
        raise ValueError(f"rerank takes candidates int64 [{Q.shape[0]}, R], R >= 1, got {cand.dtype} {tuple(cand.shape)}")
    cand = cand.to(Q.device)
    if not Q.is_cuda:
        return cpu.rerank(Q, X, cand, m)
    if Q.shape[1] > 1 and Q.stride(1) != 1:
        Q = Q.contiguous()
    if X.shape[1] > 1 and X.stride(1) != 1:
        raise ValueError("rerank takes rows with unit column stride")
    nq, R = cand.shape
    keys = torch.empty((nq, R), dtype=torch.int64, device=Q.device)
    require().rerank(Q, X, cand.contiguous(), keys)
    keys = keys.sort(dim=1).values[:, :m]
    if R >= m:
        return keys
    out = torch.full((nq, m), cpu.IVF_EMPTY_KEY, dtype=torch.int64, device=Q.device)
    out[:, :R] = keys
    return out


def pq_refine(index: PQRowIndex, Q: torch.Tensor, centers: torch.Tensor, X: torch.Tensor, m: int, nprobe: int,
              shortlist: int = INDEX_MAX_M, *, pack=None, block_queries: int | None = None) -> torch.Tensor:
    """A PQ search re-ranked on the rows: the ``m`` rows of least exact distance among the
    :func:`pq_shortlist` of every query, as :func:`rerank`'s keys ``[nq, m]``.  ``X`` ``[index.n, F]`` holds
    the rows the index was built over, in the index's dtype: on the index's device it is read in
    place; on the host (of a GPU index) every block of queries sends its candidate ids to the host
    -- one host read a block -- where the distinct rows are gathered (``index_select``), cross to the
    device once, and meet the same kernel through remapped ids: the same bits either way.  Queries
    go through in blocks (:func:`pq_refine_block_queries`, or ``block_queries``); the result does not
    depend on them."""
    m, nprobe = int(m), int(nprobe)
    if not 1 <= m <= INDEX_MAX_M:
        raise ValueError(f"search needs 1 <= m <= {INDEX_MAX_M}, got m = {m}")
    G, s = pq_shortlist_groups(shortlist)
    Qp = _search_queries(index, Q, nprobe)
    F, dev = index.F, index.codes.device
    host = X.device != dev
    if host and X.is_cuda:
        raise ValueError(f"refine takes rows on {dev} or on the host, got {X.device}")
    # (host rows of a GPU index may be of any dtype: the gathered rows are converted as they cross)
    if X.dim() != 2 or tuple(X.shape) != (index.n, F) or (X.dtype != index.dtype and not host):
        raise ValueError(f"refine takes the {index.n} indexed rows of {F} {index.dtype} features, got "
                         f"{X.dtype} {tuple(X.shape)}")
    block = (max(1, int(block_queries)) if block_queries
             else pq_refine_block_queries(index.M, nprobe, F, G * s, host_rows=host, esize=X.element_size()))
    keys = torch.empty((Qp.shape[0], m), dtype=torch.int64, device=dev)
    for s0, cand in _shortlist_blocks(index, Qp, centers, G, s, nprobe, pack, block):
        Qb = Qp[s0 : s0 + cand.shape[0], :F]
        if not host:
            keys[s0 : s0 + cand.shape[0]] = rerank(Qb, X, cand, m)
            continue
        ch = cand.cpu()                                                 # (the block's host read)
        ids = torch.unique(ch[ch >= 0])                                 # ascending: local order = row order
        staged = X.index_select(0, ids).to(device=dev, dtype=index.dtype)
        local = torch.where(ch >= 0, torch.searchsorted(ids, ch.clamp(min=0)), -1).to(dev)
        kb = rerank(Qb, staged, local, m)
        back = ids.to(dev)[(kb & 0xFFFFFFFF).clamp(max=max(ids.numel() - 1, 0))] if ids.numel() else kb
        keys[s0 : s0 + cand.shape[0]] = torch.where(kb == cpu.IVF_EMPTY_KEY, kb, (kb & ~0xFFFFFFFF) | back)
    return keys


def pq_reconstruct(index: PQRowIndex, ids: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """float32 ``[len, F]``: every id's centre plus its codewords, NaN rows for ids in no list (or out of range)."""
    n, dev, M = index.n, index.codes.device, index.M
    ids = torch.as_tensor(ids).reshape(-1).to(device=dev, dtype=torch.int64)
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    held = index.order >= 0
    at = torch.where(held, index.order, n)
    rpos = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    rpos[at] = torch.where(held, pos, -1)
    ok = (ids >= 0) & (ids < n)
    p = torch.where(ok, rpos[torch.where(ok, ids, n)], -1)
    ok = p >= 0
    p = p.clamp(min=0)
    lists = torch.bucketize(p, index.offsets[1:], right=True).clamp(max=index.K - 1)
    c = index.codes[p].to(torch.int64) if n else torch.zeros((ids.numel(), M), dtype=torch.int64, device=dev)
    words = index.codebooks[torch.arange(M, device=dev)[None, :], c]          # [len, M, dsub]
    out = centers.to(torch.float32)[lists] + words.reshape(ids.numel(), -1)
    return torch.where(ok[:, None], out, float("nan"))
