"""Plain-PyTorch reference implementations of the kernel ops (CPU path / test oracle).

Semantics match the HIP kernels exactly where it matters for tests:
* bf16 points are scored against bf16-quantised centroids, with fp32 accumulation;
* ties in the argmin go to the lowest centroid index;
* sums and counts are accumulated in float64.
"""
from __future__ import annotations

import torch

_CHUNK = 1 << 16


def quantize_centers(centers: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    c = centers.to(torch.float32)
    if dtype == torch.bfloat16:
        c = c.to(torch.bfloat16).to(torch.float32)
    return c


def row_sqnorm(X: torch.Tensor) -> torch.Tensor:
    Xf = X.to(torch.float32)
    return (Xf * Xf).sum(1)


def scores(X: torch.Tensor, centers: torch.Tensor) -> torch.Tensor:
    """``|c|^2 - 2 x.c`` in float32 (the quantity the assign kernel minimises)."""
    c = quantize_centers(centers, X.dtype)
    Xf = X.to(torch.float32)
    return (c * c).sum(1)[None, :] - 2.0 * (Xf @ c.T)


def group_norm_stats(xn: torch.Tensor, rows: int = 256) -> torch.Tensor:
    """(max, min) of ``xn`` over each ``rows``-row group, f32 [groups, 2]; the last group over its
    valid rows.  The folds start from 0 and 3e38 as the assign kernels' do (norms are >= 0)."""
    n = xn.numel()
    out = torch.empty((-(-n // rows), 2), dtype=torch.float32)
    v = xn.detach().to("cpu", torch.float32).reshape(-1)
    for gi in range(out.shape[0]):
        blk = v[gi * rows: min(n, (gi + 1) * rows)]
        out[gi, 0] = torch.clamp(blk.max(), min=0.0)
        out[gi, 1] = torch.clamp(blk.min(), max=3.0e38)
    return out


def assign(X: torch.Tensor, centers: torch.Tensor, *, with_dist: bool = True, xn=None):
    n = X.shape[0]
    labels = torch.empty(n, dtype=torch.int32, device=X.device)
    mind = torch.empty(n, dtype=torch.float32, device=X.device) if with_dist else None
    c = quantize_centers(centers, X.dtype)
    cn = (c * c).sum(1)
    for s in range(0, n, _CHUNK):
        xb = X[s : s + _CHUNK].to(torch.float32)
        sc = cn[None, :] - 2.0 * (xb @ c.T)
        m, idx = sc.min(1)
        labels[s : s + _CHUNK] = idx.to(torch.int32)
        if with_dist:
            xnb = xn[s : s + _CHUNK] if xn is not None else (xb * xb).sum(1)
            mind[s : s + _CHUNK] = (xnb + m).clamp_min(0.0)
    return labels, mind


def topk(X: torch.Tensor, centers: torch.Tensor, m: int):
    """The ``m`` nearest centres of every row: ``(idx int32 [n, m], d2 float32 [n, m])``, the
    float32 squared distances to the quantised centres ascending, equal ones by centre index
    (a stable sort)."""
    c = quantize_centers(centers, X.dtype)
    n = X.shape[0]
    idx = torch.empty((n, m), dtype=torch.int32, device=X.device)
    d2 = torch.empty((n, m), dtype=torch.float32, device=X.device)
    cn = (c * c).sum(1)
    for s in range(0, n, _CHUNK):
        xb = X[s : s + _CHUNK].to(torch.float32)
        # |x|^2 + (|c|^2 - 2 x.c), clamped: the form the kernels (and assign above) evaluate
        d = ((xb * xb).sum(1)[:, None] + (cn[None, :] - 2.0 * (xb @ c.T))).clamp_min(0.0)
        v, i = torch.sort(d, dim=1, stable=True)
        d2[s : s + _CHUNK] = v[:, :m]
        idx[s : s + _CHUNK] = i[:, :m].to(torch.int32)
    return idx, d2


QUALITY_WORDS = 24          # csrc/kernels.h QUALITY_WORDS
_MASK32 = (1 << 32) - 1


def _slot_digits(v: torch.Tensor):
    """csrc/common.h slot_add on non-negative finite float64 values: ``(j0, d)`` with the
    value truncated to a multiple of 2^-64 equal to sum_i d[i] * 2^(32 (j0 + i) - 64)
    (three 32-bit digits, int64 [3, n]; all zero for v = 0)."""
    bits = v.contiguous().view(torch.int64)
    ex = (bits >> 52) & 0x7FF
    m = (bits & ((1 << 52) - 1)) | torch.where(ex > 0, 1 << 52, 0)
    s = torch.where(ex > 0, ex, torch.ones_like(ex)) - 1075 + 64
    m = torch.where(s < 0, m >> (-s).clamp(0, 63), m)
    s = s.clamp_min(0)
    j0, o = s >> 5, s & 31
    t0 = (m & _MASK32) << o                        # < 2^63
    t1 = ((m >> 32) << o) + (t0 >> 32)
    return j0, torch.stack([t0 & _MASK32, t1 & _MASK32, t1 >> 32])


def quality_table(idx: torch.Tensor, d2: torch.Tensor, K: int) -> torch.Tensor:
    """The per-cluster quality table int64 ``[K, QUALITY_WORDS]`` of a top-1 / top-2 result
    (``idx`` int32, ``d2`` float32, both ``[n, 1 or 2]``): csrc/quality.hip in integer torch
    arithmetic, word for word (its header has the layout).  The CPU path and the test oracle."""
    if idx.dim() != 2 or idx.shape != d2.shape or idx.shape[1] not in (1, 2):
        raise ValueError(f"quality_table needs idx and d2 of one shape [n, 1 or 2], got {tuple(idx.shape)}, "
                         f"{tuple(d2.shape)}")
    QW = QUALITY_WORDS
    flat = torch.zeros(K * QW, dtype=torch.int64, device=idx.device)
    mx = torch.zeros(K, dtype=torch.int64, device=idx.device)
    for s0 in range(0, idx.shape[0], 1 << 20):
        k = idx[s0 : s0 + (1 << 20), 0].to(torch.int64)
        d = d2[s0 : s0 + (1 << 20)].to(torch.float32)
        ok = (k >= 0) & (k < K)
        k, d = k[ok], d[ok]
        fin = torch.isfinite(d[:, 0])
        flat.index_add_(0, k[~fin] * QW + 15, torch.ones_like(k[~fin]))
        k, d = k[fin], d[fin]
        a2f = d[:, 0].clamp_min(0.0) + 0.0            # (-0 -> +0)
        a2 = a2f.to(torch.float64)
        base = k * QW
        flat.index_add_(0, base + 7, torch.ones_like(k))
        for off, v in ((0, a2), (8, a2.sqrt())):
            j0, dg = _slot_digits(v)
            for i in range(3):
                flat.index_add_(0, base + off + j0 + i, dg[i])
        if d.shape[1] == 2:
            b2f = d[:, 1]
            b2 = b2f.to(torch.float64)
            sv = (1.0 - (a2 / b2).sqrt()).clamp_min(0.0)
            sv = torch.where(torch.isinf(b2f), torch.ones_like(sv), sv)
            sv = torch.where(b2f > 0, sv, torch.zeros_like(sv))          # (a NaN or zero b^2: s = 0)
            flat.index_add_(0, base + 16, torch.round(sv * 2147483648.0).to(torch.int64))
        mx.scatter_reduce_(0, k, a2f.contiguous().view(torch.int32).to(torch.int64), "amax")
    table = flat.view(K, QW)
    table[:, 17] = mx
    return table


EXEMPLAR_MAX = 64           # csrc/kernels.h EXEMPLAR_MAX
EXEMPLAR_EMPTY = -1         # the all-ones word: above every key in unsigned order
_EX_FAR = 0x7F7FFFFF        # bits of the largest finite float
_EX_LAST = (1 << 63) - 1    # stands in for the empty word while sorting (every key is below 2^63 - 2^32)


def _exemplar_smallest(keys: torch.Tensor, m: int) -> torch.Tensor:
    """Per row of int64 ``[K, w]`` keys, the ``m`` smallest distinct ones in unsigned order
    (ascending, padded with the empty word)."""
    K = keys.shape[0]
    s = torch.where(keys == EXEMPLAR_EMPTY, _EX_LAST, keys).sort(dim=1).values
    dup = torch.zeros_like(s, dtype=torch.bool)
    dup[:, 1:] = s[:, 1:] == s[:, :-1]
    s = torch.where(dup, _EX_LAST, s).sort(dim=1).values[:, :m]
    if s.shape[1] < m:
        s = torch.cat([s, torch.full((K, m - s.shape[1]), _EX_LAST, dtype=torch.int64, device=s.device)], 1)
    return torch.where(s == _EX_LAST, EXEMPLAR_EMPTY, s)


def exemplar_merge(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """Per cluster, the m smallest keys of the union of two exemplar tables (int64 ``[K, m]``)
    in unsigned order: what accumulating both tables' rows into one gives."""
    if a.shape != b.shape or a.dim() != 2:
        raise ValueError(f"exemplar_merge needs two [K, m] tables, got {tuple(a.shape)} and {tuple(b.shape)}")
    return _exemplar_smallest(torch.cat([a, b], 1), a.shape[1])


def exemplar_table(idx: torch.Tensor, d2: torch.Tensor, K: int, m: int, row0: int = 0,
                   farthest: bool = False) -> torch.Tensor:
    """The per-cluster exemplar table int64 ``[K, m]`` of a top-m result (``idx`` int32, ``d2``
    float32, both ``[n, m_topk]``, column 0 read): csrc/exemplars.hip in integer torch
    arithmetic (its header has the key layout).  Slot j of cluster k holds the (j+1)-th smallest
    key ``hi << 32 | (row0 + row)`` among the rows labelled k with a finite distance, -1 where
    the cluster has fewer.  The CPU path and the test oracle."""
    if idx.dim() != 2 or idx.shape != d2.shape or idx.shape[1] < 1:
        raise ValueError(f"exemplar_table needs idx and d2 of one shape [n, m_topk], got {tuple(idx.shape)}, "
                         f"{tuple(d2.shape)}")
    m, row0 = int(m), int(row0)
    if not 1 <= m <= EXEMPLAR_MAX:
        raise ValueError(f"exemplar_table needs 1 <= m <= {EXEMPLAR_MAX}, got m = {m}")
    if row0 < 0 or row0 + idx.shape[0] > 1 << 32:
        raise ValueError("exemplar_table takes row indices below 2^32 (row0 + n)")
    table = torch.full((K, m), EXEMPLAR_EMPTY, dtype=torch.int64, device=idx.device)
    for s0 in range(0, idx.shape[0], 1 << 20):
        k = idx[s0 : s0 + (1 << 20), 0].to(torch.int64)
        d = d2[s0 : s0 + (1 << 20), 0].to(torch.float32)
        row = torch.arange(s0, s0 + k.shape[0], dtype=torch.int64, device=idx.device) + row0
        ok = (k >= 0) & (k < K) & torch.isfinite(d)
        k, d, row = k[ok], d[ok], row[ok]
        bits = (d.clamp_min(0.0) + 0.0).contiguous().view(torch.int32).to(torch.int64)   # (-0 -> +0)
        key = ((_EX_FAR - bits if farthest else bits) << 32) | row
        o = torch.argsort(key)                         # by key, then (stable) by cluster
        o = o[torch.argsort(k[o], stable=True)]
        k, key = k[o], key[o]
        first = torch.cumsum(torch.bincount(k, minlength=K), 0) - torch.bincount(k, minlength=K)
        rank = torch.arange(k.shape[0], dtype=torch.int64, device=idx.device) - first[k]
        keep = rank < m
        part = torch.full((K, m), EXEMPLAR_EMPTY, dtype=torch.int64, device=idx.device)
        part[k[keep], rank[keep]] = key[keep]
        table = part if s0 == 0 else exemplar_merge(table, part)
    return table


QUANTILE_MAX_Q = 8          # csrc/kernels.h QUANTILE_MAX_Q
QUANTILE_BINS = 256         # one 8-bit digit
QUANTILE_PASSES = 4         # shift 24, 16, 8, 0


def quantile_hist(idx: torch.Tensor, d2: torch.Tensor, K: int, prefix: torch.Tensor | None, pass_: int) -> torch.Tensor:
    """One radix-select pass's digit histogram of a top-m result (``idx`` int32, ``d2`` float32,
    both ``[n, m_topk]``, column 0 read): csrc/quantiles.hip in integer torch arithmetic (its
    header has the passes).  Pass 0: int64 ``[K, 256]``, a row labelled k with a finite distance
    adds one to ``(k, bits >> 24)``, ``bits`` the bit pattern of max(d2, +0).  Passes 1..3
    (``prefix`` int32 ``[K, Q]``): int64 ``[K, Q, 256]``, the row adds one to
    ``(k, j, (bits >> s) & 255)`` for every j whose prefix shares its bits above ``s + 8``,
    ``s = 24 - 8 * pass``.  The CPU path and the test oracle."""
    if idx.dim() != 2 or idx.shape != d2.shape or idx.shape[1] < 1:
        raise ValueError(f"quantile_hist needs idx and d2 of one shape [n, m_topk], got {tuple(idx.shape)}, "
                         f"{tuple(d2.shape)}")
    pass_, K = int(pass_), int(K)
    if not 0 <= pass_ < QUANTILE_PASSES:
        raise ValueError(f"quantile_hist needs a pass in 0..3, got {pass_}")
    if pass_ and (prefix is None or prefix.dim() != 2 or prefix.shape[0] != K
                  or not 1 <= prefix.shape[1] <= QUANTILE_MAX_Q):
        raise ValueError(f"quantile_hist needs a [K, Q] prefix with 1 <= Q <= {QUANTILE_MAX_Q} in passes 1..3")
    Q = prefix.shape[1] if pass_ else 1
    s = 24 - 8 * pass_
    flat = torch.zeros(K * Q * QUANTILE_BINS, dtype=torch.int64, device=idx.device)
    for s0 in range(0, idx.shape[0], 1 << 20):
        k = idx[s0 : s0 + (1 << 20), 0].to(torch.int64)
        d = d2[s0 : s0 + (1 << 20), 0].to(torch.float32)
        ok = (k >= 0) & (k < K) & torch.isfinite(d)
        k, d = k[ok], d[ok]
        bits = (d.clamp_min(0.0) + 0.0).contiguous().view(torch.int32).to(torch.int64)   # (-0 -> +0)
        digit = (bits >> s) & 255
        if pass_ == 0:
            flat += torch.bincount(k * QUANTILE_BINS + digit, minlength=flat.shape[0])
            continue
        for j in range(Q):
            hit = (bits >> (s + 8)) == (prefix[k, j].to(torch.int64) >> (s + 8))
            flat += torch.bincount(((k * Q + j) * QUANTILE_BINS + digit)[hit], minlength=flat.shape[0])
    return flat.view(K, QUANTILE_BINS) if pass_ == 0 else flat.view(K, Q, QUANTILE_BINS)


def quantile_select(table: torch.Tensor, q: torch.Tensor, prefix: torch.Tensor, rank: torch.Tensor, pass_: int):
    """One select step on a summed histogram: ``(prefix int32 [K, Q], rank int64 [K, Q], counts
    int64 [K] or None)``.  Pass 0 (``table`` ``[K, 256]``; ``prefix`` and ``rank`` give the shape
    only): ``counts`` = n_k, r = clamp(ceil(q * n_k) - 1, 0, n_k - 1) with the product one float64
    multiply, b the smallest bin whose running count exceeds r, prefix = b << 24 and rank = r - the
    count below b.  Passes 1..3 (``[K, Q, 256]``): the same from the given rank, prefix |= b << s.
    A pair whose bins hold no more than its rank (an empty cluster) keeps prefix and rank (zeros
    from pass 0)."""
    pass_ = int(pass_)
    K, Q = prefix.shape
    s = 24 - 8 * pass_
    counts = None
    if pass_ == 0:
        counts = table.sum(1)
        r = torch.ceil(q.to(torch.float64)[None, :] * counts.to(torch.float64)[:, None]).to(torch.int64) - 1
        R = torch.minimum(r, counts[:, None] - 1).clamp_min(0)
        H = table[:, None, :].expand(K, Q, QUANTILE_BINS)
        P = torch.zeros((K, Q), dtype=torch.int64, device=table.device)
        keepR = torch.zeros_like(R)
    else:
        R, H, P = rank.to(torch.int64), table, prefix.to(torch.int64)
        keepR = R
    cum = H.cumsum(-1)
    over = cum > R[..., None]
    has = over.any(-1)
    b = over.to(torch.int8).argmax(-1)                      # the first bin past the rank
    below = (cum - H).gather(-1, b[..., None])[..., 0]
    P = torch.where(has, P | (b << s), P)
    R = torch.where(has, R - below, keepR)
    return P.to(torch.int32), R, counts


def cluster_sums(X: torch.Tensor, labels: torch.Tensor, K: int, weights=None):
    lab = labels.to(torch.int64)
    Xd = X.to(torch.float64)
    if weights is not None:
        w = weights.to(torch.float64)
        Xd = Xd * w[:, None]
        counts = torch.zeros(K, dtype=torch.float64, device=X.device).index_add_(0, lab, w)
    else:
        counts = torch.bincount(lab, minlength=K).to(torch.float64)
    sums = torch.zeros((K, X.shape[1]), dtype=torch.float64, device=X.device).index_add_(0, lab, Xd)
    return sums, counts


PARTITION_MAX_K = 10240             # csrc/kernels.h PARTITION_MAX_K (the native partition's largest K)
IVF_EMPTY_KEY = (1 << 63) - 1       # csrc/kernels.h IVF_EMPTY_KEY: a search slot without a row
PAD_SCORE = 1.0e30                  # csrc/common.h PAD_SCORE: cn of a pad row


def partition(labels: torch.Tensor, K: int):
    """``(order, offsets, rpos)`` of a stable partition of the rows by label (csrc/ivf.hip in torch
    arithmetic): ``order`` int64 [n] = the rows whose label lies in [0, K), label after label and
    ascending within a label (a stable sort), tail -1; ``offsets`` int64 [K + 1] the cumulative
    bincount; ``rpos`` int64 [n] every row's position in ``order``, -1 for a row in no list."""
    lab = labels.to(torch.int64)
    n, dev = lab.numel(), lab.device
    rows = ((lab >= 0) & (lab < K)).nonzero().flatten()
    kept = lab[rows]
    perm = torch.sort(kept, stable=True).indices
    order = torch.full((n,), -1, dtype=torch.int64, device=dev)
    order[: rows.numel()] = rows[perm]
    offsets = torch.zeros(K + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(torch.bincount(kept, minlength=K), 0)
    rpos = torch.full((n,), -1, dtype=torch.int64, device=dev)
    rpos[rows[perm]] = torch.arange(rows.numel(), dtype=torch.int64, device=dev)
    return order, offsets, rpos


def index_pack(X: torch.Tensor, row0: int, labels: torch.Tensor, rpos: torch.Tensor, offsets: torch.Tensor,
               toff: torch.Tensor, rows_out: torch.Tensor, cn: torch.Tensor) -> None:
    """Rows [row0, row0 + nb) of an index into its natural-layout row store ``rows_out``
    ([16 tiles, cols]) and ``cn`` (their squared norms): row i lands at
    ``16 toff[k] + rpos[i] - offsets[k]``, k its list (csrc/ivf.hip's row pack without the
    fragment layout)."""
    nb = X.shape[0]
    p = rpos[row0 : row0 + nb]
    ok = p >= 0
    k = labels[row0 : row0 + nb][ok].to(torch.int64)
    dst = toff[k] * 16 + p[ok] - offsets[k]
    x = X[ok]
    rows_out[dst, : X.shape[1]] = x
    xf = x.to(torch.float32)
    cn[dst] = (xf * xf).sum(1)


def index_repack(rows_old: torch.Tensor, cn_old: torch.Tensor, offsets_old: torch.Tensor, toff_old: torch.Tensor,
                 rpos_old: torch.Tensor, labels: torch.Tensor, rpos: torch.Tensor, offsets: torch.Tensor,
                 toff: torch.Tensor, rows_out: torch.Tensor, cn: torch.Tensor) -> None:
    """The rows that stay in an updated index, from its old natural-layout row store into the new
    one (csrc/ivf.hip's repack without the fragment layout): every id below ``rpos_old.numel()``
    with a list in ``labels`` moves from ``16 toff_old[k] + rpos_old[id] - offsets_old[k]`` to
    ``16 toff[k] + rpos[id] - offsets[k]``, its row and its ``cn`` as stored."""
    n_old = rpos_old.numel()
    lab = labels[:n_old].to(torch.int64)
    ids = ((lab >= 0) & (rpos_old >= 0)).nonzero().flatten()
    k = lab[ids]
    src = toff_old[k] * 16 + rpos_old[ids] - offsets_old[k]
    dst = toff[k] * 16 + rpos[ids] - offsets[k]
    rows_out[dst] = rows_old[src]
    cn[dst] = cn_old[src]


def _index_rows(index, D: int):
    """The indexed rows in list order: ``(lid, rid, c, cn)`` -- every position's list and row id, the
    rows themselves (float32, ``D`` columns) and their squared norms, gathered from the pack's tiles."""
    K, dev = index.K, index.order.device
    sizes = index.offsets[1:] - index.offsets[:-1]
    nv = int(index.offsets[K])
    lid = torch.repeat_interleave(torch.arange(K, dtype=torch.int64, device=dev), sizes)       # list of position p
    slot = index.tile_offsets[lid] * 16 + torch.arange(nv, dtype=torch.int64, device=dev) - index.offsets[lid]
    store = index.pack.view(-1, index.cols)
    return lid, index.order[:nv], store[slot][:, :D].to(torch.float32), index.cn[slot]


def _block_d2(Qb: torch.Tensor, c: torch.Tensor, cn: torch.Tensor) -> torch.Tensor:
    """Clamped squared distances [queries, rows] of a block of queries, in :func:`topk`'s form."""
    xb = Qb.to(torch.float32)
    return ((xb * xb).sum(1)[:, None] + (cn[None, :] - 2.0 * (xb @ c.T))).clamp_min(0.0) + 0.0   # (-0 -> +0)


def index_search(index, Q: torch.Tensor, centers: torch.Tensor, m: int, nprobe: int) -> torch.Tensor:
    """Sorted search keys int64 [nq, m] (``d2 bits << 32 | row``, ``IVF_EMPTY_KEY`` padded) over
    the lists of every query's ``nprobe`` nearest centres (:func:`topk`'s indices).  ``d2`` is
    :func:`topk`'s form with the indexed rows in the place of the centres."""
    K, dev, nq = index.K, Q.device, Q.shape[0]
    lid, rid, c, cn = _index_rows(index, Q.shape[1])
    probes = topk(Q, centers, nprobe)[0].to(torch.int64)
    keys = torch.full((nq, m), IVF_EMPTY_KEY, dtype=torch.int64, device=dev)
    rows = max(1, (1 << 24) // max(rid.numel(), 1))
    for s in range(0, nq, rows):
        d = _block_d2(Q[s : s + rows], c, cn)
        key = (d.contiguous().view(torch.int32).to(torch.int64) << 32) | rid[None, :]
        member = torch.zeros((d.shape[0], K), dtype=torch.bool, device=dev)
        member.scatter_(1, probes[s : s + rows], True)
        key = torch.where(member[:, lid], key, IVF_EMPTY_KEY).sort(dim=1).values[:, :m]
        keys[s : s + rows, : key.shape[1]] = key
    return keys


def index_range(index, Q: torch.Tensor, centers: torch.Tensor, r2: torch.Tensor, nprobe: int, *, sort: bool = True,
                count_only: bool = False, want_probe: bool = False):
    """Range search in the arithmetic of :func:`index_search`: ``(lims int64 [nq + 1], keys int64
    [total])``, query q's hits -- the rows of its ``nprobe`` probed lists with ``d2 <= r2[q]`` -- as
    ``d2 bits << 32 | row`` keys in ``keys[lims[q]:lims[q + 1]]``: ascending (``sort``), or probe
    after probe and in list order within a probe.  ``count_only``: ``counts int64 [nq]`` alone;
    ``want_probe``: also every hit's probe rank.  ``r2``: float32 [nq], finite and non-negative (a
    NaN or infinite ``d2`` is no hit)."""
    K, dev, nq = index.K, Q.device, Q.shape[0]
    lid, rid, c, cn = _index_rows(index, Q.shape[1])
    probes = topk(Q, centers, nprobe)[0].to(torch.int64) if nq else torch.zeros((0, nprobe), dtype=torch.int64, device=dev)
    counts = torch.zeros(nq, dtype=torch.int64, device=dev)
    keys, ranks = [], []
    rows = max(1, (1 << 24) // max(rid.numel(), 1))
    for s in range(0, nq, rows):
        d = _block_d2(Q[s : s + rows], c, cn)
        prank = torch.full((d.shape[0], K), nprobe, dtype=torch.int64, device=dev)            # a list's probe rank
        prank.scatter_(1, probes[s : s + rows], torch.arange(nprobe, dtype=torch.int64, device=dev).expand(d.shape[0], -1))
        pr = prank[:, lid]
        hit = (pr < nprobe) & (d <= r2[s : s + rows, None])
        counts[s : s + rows] = hit.sum(1)
        if count_only:
            continue
        q, p = hit.nonzero(as_tuple=True)                                                      # query-major, list order
        key = (d[q, p].contiguous().view(torch.int32).to(torch.int64) << 32) | rid[p]
        pr = pr[q, p]
        if sort:
            key, o1 = key.sort()
            o2 = q[o1].sort(stable=True).indices
            key, pr = key[o2], pr[o1][o2]
        else:
            o = (q * nprobe + pr).sort(stable=True).indices                                    # pair after pair
            key, pr = key[o], pr[o]
        keys.append(key)
        ranks.append(pr)
    if count_only:
        return counts
    lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
    lims[1:] = torch.cumsum(counts, 0)
    empty = torch.zeros(0, dtype=torch.int64, device=dev)
    keys = torch.cat(keys) if keys else empty
    if want_probe:
        return lims, keys, (torch.cat(ranks) if ranks else empty)
    return lims, keys


INDEX_DEEP_MAX_M = 2048             # csrc/kernels.h IVF_DEEP_MAX_M: the longest deep-search result


def index_pair_bits(index, Q: torch.Tensor, probes: torch.Tensor):
    """What a deep search ranks, in the arithmetic of :func:`index_search`: ``(bits int64 [nq, nv],
    member bool [nq, nv], rid int64 [nv])`` -- the bit pattern of every query's ``d2`` against every
    indexed row (in list order), whether the row's list is one of the query's ``probes`` (int
    [nq, nprobe]) and the rows' ids."""
    lid, rid, c, cn = _index_rows(index, Q.shape[1])
    bits = _block_d2(Q, c, cn).contiguous().view(torch.int32).to(torch.int64)
    member = torch.zeros((Q.shape[0], index.K), dtype=torch.bool, device=Q.device)
    member.scatter_(1, probes.to(torch.int64), True)
    return bits, member[:, lid], rid


def index_hist(bits: torch.Tensor, member: torch.Tensor, prefix: torch.Tensor | None, pass_: int) -> torch.Tensor:
    """One radix-select pass's histogram of a deep search (csrc/deep.hip ivf_hist_kernel in integer
    torch arithmetic): int64 ``[nq, 256]``.  ``bits`` int64 ``[nq, nc]``: the bit patterns of every
    query's clamped ``d2`` against ``nc`` candidate rows; ``member`` bool ``[nq, nc]``: the rows
    that count for the query (those of its probed lists).  Pass 0: a row adds one to
    ``(q, bits >> 24)``; passes 1..3 (``prefix`` int32 ``[nq]``): to ``(q, (bits >> s) & 255)`` where
    ``bits >> (s + 8) == prefix[q] >> (s + 8)``, ``s = 24 - 8 * pass``.  No finiteness filter."""
    pass_ = int(pass_)
    if not 0 <= pass_ < QUANTILE_PASSES:
        raise ValueError(f"index_hist needs a pass in 0..3, got {pass_}")
    if pass_ and (prefix is None or prefix.shape != bits.shape[:1]):
        raise ValueError("index_hist needs a prefix [nq] in passes 1..3")
    nq, s = bits.shape[0], 24 - 8 * pass_
    ok = member
    if pass_:
        ok = ok & ((bits >> (s + 8)) == ((prefix.to(torch.int64) & 0xFFFFFFFF) >> (s + 8))[:, None])
    slot = torch.arange(nq, dtype=torch.int64, device=bits.device)[:, None] * QUANTILE_BINS + ((bits >> s) & 255)
    return torch.bincount(slot[ok], minlength=nq * QUANTILE_BINS).view(nq, QUANTILE_BINS)


def index_select(table: torch.Tensor, prefix: torch.Tensor, rank: torch.Tensor, cand: torch.Tensor, m: int, pass_: int):
    """One select step of a deep search on a histogram int64 ``[nq, 256]`` (csrc/deep.hip
    ivf_select_kernel): ``(prefix int32 [nq], rank int64 [nq], hits int64 [nq], cand int64 [nq])``.
    Pass 0 (``prefix``, ``rank`` and ``cand`` are not read): ``cand`` = the sum of the bins and
    R = min(m, cand) - 1; later passes R = ``rank``.  b = the smallest bin whose running count
    exceeds R: prefix |= b << s, rank = R - the count below b and hits = the candidates with
    ``bits <= prefix | (2^s - 1)`` = min(m, cand) - 1 - rank + count[b].  ``cand`` = 0: all zeros."""
    pass_, m = int(pass_), int(m)
    s = 24 - 8 * pass_
    if pass_ == 0:
        cand = table.sum(1)
        P = torch.zeros_like(cand)
    else:
        P = prefix.to(torch.int64) & 0xFFFFFFFF
    found = cand.clamp(max=m)
    R = found - 1 if pass_ == 0 else rank.to(torch.int64)
    cum = table.cumsum(1)
    over = cum > R[:, None]
    has = over.any(1) & (cand > 0)                           # (false only where cand = 0)
    b = over.to(torch.int8).argmax(1)
    below = (cum - table).gather(1, b[:, None])[:, 0]
    zero = torch.zeros_like(R)
    P = torch.where(has, P | (b << s), zero)
    R = torch.where(has, R - below, zero)
    hits = torch.where(has, found - 1 - R + table.gather(1, b[:, None])[:, 0], zero)
    return P.to(torch.int32), R, hits, cand


# ---- product-quantised index (csrc/pq.hip, csrc/pqplan.h) ----------------------------------------
PQ_SUBVECTORS = (8, 16, 32, 64)     # csrc/pqplan.h pq_subvectors_ok
PQ_KSUB = 256                       # codewords of a sub-space
PQ_MAX_SPLITS = 8                   # csrc/pqplan.h PQ_MAX_SPLITS


def pq_encode(R: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """Codes uint8 ``[n, M]``: sub-vector j's nearest codeword by :func:`topk` (m = 1)."""
    M, _, dsub = codebooks.shape
    codes = torch.empty((R.shape[0], M), dtype=torch.uint8, device=R.device)
    for j in range(M):
        codes[:, j] = topk(R[:, j * dsub : (j + 1) * dsub], codebooks[j].to(R.device), 1)[0][:, 0].to(torch.uint8)
    return codes


def pq_lut(RQ: torch.Tensor, codebooks: torch.Tensor) -> torch.Tensor:
    """Tables float32 ``[npairs, M, 256]``: sub-vector j's squared distances to the quantised codewords,
    in the form :func:`mikmeans.ops.transform` takes off the GPU (``cdist``, squared)."""
    M, _, dsub = codebooks.shape
    lut = torch.empty((RQ.shape[0], M, PQ_KSUB), dtype=torch.float32, device=RQ.device)
    for j in range(M):
        d = torch.cdist(RQ[:, j * dsub : (j + 1) * dsub].to(torch.float32),
                        quantize_centers(codebooks[j].to(RQ.device), RQ.dtype))
        lut[:, j, :] = d * d
    return lut


def pq_adc(lut: torch.Tensor, pair: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    """``lut[pair, 0, codes[:, 0]] + lut[pair, 1, codes[:, 1]] + ...``: float32 adds in sub-space order
    (csrc/pq.hip pq_adc).  ``pair`` int64 ``[nq, rows]``, ``codes`` uint8 ``[rows, M]``."""
    c = codes.to(torch.int64)
    acc = lut[pair, 0, c[None, :, 0]]
    for j in range(1, codes.shape[1]):
        acc = torch.add(acc, lut[pair, j, c[None, :, j]])
    return acc


def pq_scan(index, lut: torch.Tensor, probes: torch.Tensor, m: int) -> torch.Tensor:
    """Sorted search keys int64 ``[nq, m]`` (``ADC bits << 32 | row``, ``IVF_EMPTY_KEY`` padded) of the
    queries whose pairs ``q * nprobe + j`` have the tables ``lut`` and the lists ``probes`` ``[nq, nprobe]``."""
    K, dev = index.K, lut.device
    nq, nprobe = probes.shape
    sizes = index.offsets[1:] - index.offsets[:-1]
    nv = int(index.offsets[K])
    lid = torch.repeat_interleave(torch.arange(K, dtype=torch.int64, device=dev), sizes)
    rid, codes = index.order[:nv], index.codes[:nv]
    keys = torch.full((nq, m), IVF_EMPTY_KEY, dtype=torch.int64, device=dev)
    rows = max(1, (1 << 22) // max(nv, 1))
    for s in range(0, nq, rows):
        pr = probes[s : s + rows].to(torch.int64)
        nb = pr.shape[0]
        rank = torch.full((nb, K), -1, dtype=torch.int64, device=dev)
        rank.scatter_(1, pr, torch.arange(nprobe, dtype=torch.int64, device=dev)[None, :].expand(nb, nprobe))
        of = rank[:, lid]                                               # [nb, nv]: the probe rank of the row's list
        pair = (torch.arange(s, s + nb, dtype=torch.int64, device=dev)[:, None] * nprobe + of.clamp(min=0))
        d = pq_adc(lut, pair, codes)
        key = (d.contiguous().view(torch.int32).to(torch.int64) << 32) | rid[None, :]
        key = torch.where(of >= 0, key, IVF_EMPTY_KEY).sort(dim=1).values[:, :m]
        keys[s : s + rows, : key.shape[1]] = key
    return keys


def pq_shortlist(index, lut: torch.Tensor, probes: torch.Tensor, G: int, s: int) -> torch.Tensor:
    """Shortlist keys int64 ``[nq, nprobe, G, s]`` (``ADC bits << 32 | row``, ``IVF_EMPTY_KEY`` padded):
    position ``p`` of a probed list is in group ``(p // 256) mod G`` -- the chunks csrc/pqplan.h deals
    to split ``g`` of ``G`` -- and every group keeps its ``s`` smallest keys, ascending."""
    nq, nprobe = probes.shape
    dev = lut.device
    out = torch.full((nq, nprobe, G, s), IVF_EMPTY_KEY, dtype=torch.int64, device=dev)
    offs = index.offsets.tolist()
    pr = probes.tolist()
    for q in range(nq):
        for j in range(nprobe):
            a, b = offs[pr[q][j]], offs[pr[q][j] + 1]
            if a == b:
                continue
            pair = torch.full((1, b - a), q * nprobe + j, dtype=torch.int64, device=dev)
            d = pq_adc(lut, pair, index.codes[a:b])[0]
            key = (d.contiguous().view(torch.int32).to(torch.int64) << 32) | index.order[a:b]
            group = (torch.arange(b - a, device=dev) // 256) % G
            for g in range(min(G, (b - a + 255) // 256)):
                k = key[group == g].sort().values[:s]
                out[q, j, g, : k.numel()] = k
    return out


# ---- the re-rank of candidates against the rows (csrc/rerank.hip, csrc/rerankplan.h) ----------------
RERANK_GROUP = 16                   # csrc/rerankplan.h RR_GROUP: the accumulators of a pair


def rerank_keys(Q: torch.Tensor, X: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """Keys int64 ``[nq, R]``, ``d2 bits << 32 | cand`` and ``IVF_EMPTY_KEY`` for an id outside ``[0, n)``,
    in the order of adds of csrc/rerank.hip: pieces of ``V`` = 8 (bfloat16) or 4 columns, accumulator
    ``s`` of sixteen takes the pieces ``s, s + 16, ...`` column after column as ``d = q - x``,
    ``p = d * d``, ``a = a + p`` (``torch.sub`` / ``mul`` / ``add``: one rounding each), and the
    accumulators meet as ``((a0+a1)+(a2+a3)) + ((a4+a5)+(a6+a7))`` plus the same over ``a8..a15``."""
    nq, F = Q.shape
    n, R = X.shape[0], cand.shape[1]
    V = 8 if Q.dtype == torch.bfloat16 else 4
    G = RERANK_GROUP
    pieces = (F + V - 1) // V
    rounds = (pieces + G - 1) // G
    width = rounds * G * V
    ok = (cand >= 0) & (cand < n)
    keys = torch.empty((nq, R), dtype=torch.int64, device=Q.device)
    rows = max(1, (1 << 24) // max(R * width, 1))
    zero = torch.zeros((), dtype=torch.float32, device=Q.device)
    for s in range(0, nq, rows):
        okb = ok[s : s + rows]
        c = torch.where(okb, cand[s : s + rows], 0)
        nb = c.shape[0]
        xf = (X[c.reshape(-1)].to(torch.float32).view(nb, R, F) if n else torch.zeros((nb, R, F), device=Q.device))
        d = torch.sub(Q[s : s + rows].to(torch.float32)[:, None, :], xf)
        p = torch.zeros((nb, R, width), dtype=torch.float32, device=Q.device)   # (a column >= F: 0 - 0, squared)
        p[:, :, :F] = torch.mul(d, d)
        p = p.view(nb, R, rounds, G, V)
        a = torch.zeros((nb, R, G), dtype=torch.float32, device=Q.device)
        for k in range(rounds):
            for e in range(V):
                a = torch.add(a, p[:, :, k, :, e])
        h = [torch.add(torch.add(torch.add(a[..., o], a[..., o + 1]), torch.add(a[..., o + 2], a[..., o + 3])),
                       torch.add(torch.add(a[..., o + 4], a[..., o + 5]), torch.add(a[..., o + 6], a[..., o + 7])))
             for o in (0, 8)]
        d2 = torch.add(h[0], h[1])
        nan = torch.isnan(d2)               # (clamp_d2: one NaN pattern; a sum of squares is never negative)
        bits = torch.where(nan, 0x7FC00000, torch.where(nan, zero, d2).contiguous().view(torch.int32).to(torch.int64))
        keys[s : s + rows] = torch.where(okb, (bits << 32) | c, IVF_EMPTY_KEY)
    return keys


def rerank(Q: torch.Tensor, X: torch.Tensor, cand: torch.Tensor, m: int) -> torch.Tensor:
    """The ``m`` smallest of :func:`rerank_keys` per query, ascending, ``IVF_EMPTY_KEY`` padded."""
    keys = rerank_keys(Q, X, cand).sort(dim=1).values[:, :m]
    if keys.shape[1] == m:
        return keys
    out = torch.full((Q.shape[0], m), IVF_EMPTY_KEY, dtype=torch.int64, device=Q.device)
    out[:, : keys.shape[1]] = keys
    return out
