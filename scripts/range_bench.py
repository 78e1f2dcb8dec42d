"""range_search / range_count beside search on the GPU: one process, device-event times of warm
calls, the three interleaved.

bf16 blobs, D = 128, K centres from a short fit; every query's radius is its 10th-neighbour
distance (``search(Q, 10, nprobe)``'s last column), so a query has ten hits or, on ties, more.  It
prints one JSON record: the median (min .. max) of ``range_search``, ``range_count`` and ``search``
over ``--repeats`` rounds, the total hit count, and where the range search's time goes (the probes,
the partition of the pairs, the count pass, the cumulative sum with its host read, the fill pass,
the per-query sort).

Usage: ``python scripts/range_bench.py [--n 2000000] [--k 1024] [--nq 10000] [--nprobe 16] [--m 10]
[--repeats 20]``
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mikmeans  # noqa: E402
from mikmeans import ops  # noqa: E402
from mikmeans.data import blobs as B  # noqa: E402
from mikmeans.ops.native import dtype_code  # noqa: E402

D = 128


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def phases(index, Q, C, pk, r2, nprobe, repeats):
    """The steps of ``ops.index_range`` on one block of queries, each timed on its own."""
    ext = ops.require()
    nq = Q.shape[0]
    npairs = nq * nprobe
    t = {k: [] for k in ("probes", "partition", "count", "cumsum_read", "fill", "sort")}
    for r in range(repeats + 1):
        (probes, _), a = _timed(lambda: ops.topk(Q, C, nprobe, pack=pk))

        P = ext.ivf_range_blocks(dtype_code(Q.dtype), index.cols, npairs)
        (porder, poff, icum, max_items), b = _timed(lambda: ops.pair_items(index, probes, P))
        counts = torch.zeros(npairs, dtype=torch.int64, device=Q.device)
        args = (Q, ops.row_sqnorm(Q), r2, index.pack, index.cn, index.offsets, index.tile_offsets, index.order, porder,
                poff, icum, nprobe, index.cols, P, max_items, counts)
        _, c = _timed(lambda: ext.ivf_range(*args))

        def scan():
            end = torch.cumsum(counts, 0)
            return end, torch.empty(int(end[-1]), dtype=torch.int64, device=Q.device)

        (end, keys), d = _timed(scan)
        _, e = _timed(lambda: ext.ivf_range(*args, end - counts, keys))

        def order():
            qid = torch.repeat_interleave(torch.arange(nq, device=Q.device), counts.view(nq, nprobe).sum(1),
                                          output_size=keys.numel())
            ks, o1 = keys.sort()
            return ks[qid[o1].sort(stable=True).indices]

        _, f = _timed(order)
        if r:
            for k, v in zip(t, (a, b, c, d, e, f)):
                t[k].append(v)
    return {k: _stat(v) for k, v in t.items()}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--m", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("range_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    K, m, nprobe = a.k, a.m, a.nprobe
    X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
    km = mikmeans.KMeans(K, dtype="bfloat16", init="random", max_iter=3, seed=0).fit(X[: min(a.n, 1 << 20)])
    index = km.build_index(X)
    g = torch.Generator(device="cpu").manual_seed(11)
    Q = (X[torch.randint(0, a.n, (a.nq,), generator=g).to(dev)].float()
         + 0.5 * torch.randn(a.nq, D, generator=g).to(dev)).to(torch.bfloat16)
    _, d2 = index.search(Q, m, nprobe=nprobe, squared=True)
    r2 = torch.nan_to_num(d2[:, m - 1], nan=0.0).contiguous()          # (a query with fewer than m rows probed: 0)
    t = {"range_search": [], "range_count": [], "search": []}
    for r in range(a.repeats + 1):                                     # (the first round warms every code object)
        (lims, rows, dist), ta = _timed(lambda: index.range_search(Q, r2, nprobe=nprobe, squared=True))
        counts, tb = _timed(lambda: index.range_count(Q, r2, nprobe=nprobe, squared=True))
        (srows, sd2), tc = _timed(lambda: index.search(Q, m, nprobe=nprobe, squared=True))
        if r:
            for k, v in zip(t, (ta, tb, tc)):
                t[k].append(v)
    assert torch.equal(counts, lims[1:] - lims[:-1])
    full = srows[:, m - 1] >= 0
    first = lims[:-1, None] + torch.arange(m, device=dev)[None, :]
    assert bool((counts[full] >= m).all()) and torch.equal(rows[first[full]], srows[full])
    pk = km._serving_pack(Q)
    rec = {"what": "range", "n": a.n, "D": D, "K": K, "nq": a.nq, "nprobe": nprobe, "m": m,
           **{k: _stat(v) for k, v in t.items()}, "hits": int(lims[-1]), "queries_with_m_rows": int(full.sum()),
           "phases": phases(index._index, Q, km.cluster_centers_, pk, r2, nprobe, min(a.repeats, 5))}
    print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
