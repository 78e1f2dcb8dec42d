"""search_deep beside search and range_search on the GPU: one process, device-event times of warm
calls, interleaved.

bf16 blobs, D = 128, K centres from a short fit.  For every ``m`` of ``--m`` it times
``search_deep(Q, m)`` against two references: ``search(Q, 32)`` (the scan kernel's register list)
and ``range_search`` with every query's true m-th distance as its radius -- count, fill and sort
alone, the floor a method that has to find that radius first cannot beat.  It prints one JSON record
per ``m``: the medians (min .. max) over ``--repeats`` rounds, the passes the stop rule took, the
whole call at every forced pass count, and where the time goes: every histogram pass, the selects,
the count pass, the cumulative sum with its host read, the fill pass, the sort and cut to ``m`` --
with the ratios of each histogram pass to the count pass and of ``search_deep`` to the scan.

Usage: ``python scripts/search_deep_bench.py [--n 2000000] [--k 1024] [--nq 10000] [--nprobe 16]
[--m 32 100 1000] [--repeats 20]``
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
from mikmeans.ops import index as iops  # noqa: E402
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


def phases(index, Q, C, pk, m, nprobe, repeats):
    """The steps of ``ops.index_search_deep`` on one block of queries, each timed on its own; all
    four histogram passes run, whatever the stop rule would do."""
    ext = ops.require()
    nq, dev = Q.shape[0], Q.device
    npairs = nq * nprobe
    probes, _ = ops.topk(Q, C, nprobe, pack=pk)
    PH = ext.ivf_hist_blocks(dtype_code(Q.dtype), index.cols, npairs)
    walks = {P: iops._walk_args(index, Q, probes, P) for P in sorted({1, PH})}
    r2, took = iops._deep_radius(index, Q, probes, m, None)
    t = {}
    for r in range(repeats + 1):
        row = {}
        prefix = torch.zeros(nq, dtype=torch.int32, device=dev)
        rank, hits, cand = (torch.zeros(nq, dtype=torch.int64, device=dev) for _ in range(3))
        table = torch.zeros((nq, 256), dtype=torch.int32, device=dev)
        over = []
        for p in range(4):
            for P, walk in walks.items():
                table.zero_()
                _, row[f"hist{p}_P{P}"] = _timed(lambda: ext.ivf_hist(*walk, table, prefix if p else None, p))
            _, row[f"select{p}"] = _timed(lambda: ext.ivf_select(table, prefix, rank, hits, cand, m, p))
            over.append(float(hits.sum()) / max(1.0, float(cand.clamp(max=m).sum())))
        PR = ext.ivf_range_blocks(dtype_code(Q.dtype), index.cols, npairs)
        counts = torch.zeros(npairs, dtype=torch.int64, device=dev)
        args = (*iops._walk_args(index, Q, probes, PR, r2), counts)
        _, row["count"] = _timed(lambda: ext.ivf_range(*args))

        def scan():
            end = torch.cumsum(counts, 0)
            return end, torch.empty(int(end[-1]), dtype=torch.int64, device=dev)

        (end, keys), row["cumsum_read"] = _timed(scan)
        _, row["fill"] = _timed(lambda: ext.ivf_range(*args, end - counts, keys))

        def cut():
            cq = counts.view(nq, nprobe).sum(1)
            qid = torch.repeat_interleave(torch.arange(nq, device=dev), cq, output_size=keys.numel())
            ks, o1 = keys.sort()
            o2 = qid[o1].sort(stable=True).indices
            ks, qs = ks[o2], qid[o1][o2]
            pos = torch.arange(ks.numel(), device=dev) - (torch.cumsum(cq, 0) - cq)[qs]
            keep = pos < m
            out = torch.full((nq, m), ops.IVF_EMPTY_KEY, dtype=torch.int64, device=dev)
            out[qs[keep], pos[keep]] = ks[keep]
            return out

        _, row["sort_cut"] = _timed(cut)
        if r:
            for k, v in row.items():
                t.setdefault(k, []).append(v)
    out = {k: _stat(v) for k, v in t.items()}
    count = out["count"]["median_ms"]
    return {"hist_blocks": PH, "range_blocks": PR, "passes_taken": took, "keys_collected": int(keys.numel()),
            "hits_over_found_after_pass": [round(x, 3) for x in over], "phases": out,
            "hist_over_count": {k: round(v["median_ms"] / count, 3) for k, v in out.items() if k.startswith("hist")}}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--n", type=int, default=2_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=10_000)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--m", type=int, nargs="+", default=[32, 100, 1000])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("search_deep_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    K, nprobe = a.k, a.nprobe
    X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
    km = mikmeans.KMeans(K, dtype="bfloat16", init="random", max_iter=3, seed=0).fit(X[: min(a.n, 1 << 20)])
    index = km.build_index(X)
    g = torch.Generator(device="cpu").manual_seed(11)
    Q = (X[torch.randint(0, a.n, (a.nq,), generator=g).to(dev)].float()
         + 0.5 * torch.randn(a.nq, D, generator=g).to(dev)).to(torch.bfloat16)
    pk = km._serving_pack(Q)
    for m in a.m:
        rows, d2 = index.search_deep(Q, m, nprobe=nprobe, squared=True)
        found = (rows >= 0).sum(1)
        last = d2.gather(1, (found - 1).clamp_min(0)[:, None])[:, 0]
        r2 = torch.where(found > 0, last, 0.0).contiguous()             # every query's true m-th distance
        t = {"search_deep": [], "range_search": [], "search_32": []}
        for r in range(a.repeats + 1):                                 # (the first round warms every code object)
            (drows, dd2), ta = _timed(lambda: index.search_deep(Q, m, nprobe=nprobe, squared=True))
            (lims, rrows, _), tb = _timed(lambda: index.range_search(Q, r2, nprobe=nprobe, squared=True))
            (srows, sd2), tc = _timed(lambda: index.search(Q, 32, nprobe=nprobe, squared=True))
            if r:
                for k, v in zip(t, (ta, tb, tc)):
                    t[k].append(v)
        forced = {p: [] for p in (1, 2, 3, 4)}                         # what INDEX_DEEP_OVERSHOOT trades
        for r in range(min(a.repeats, 5) + 1):
            for p in forced:
                (frows, _), tp = _timed(lambda: index.search_deep(Q, m, nprobe=nprobe, squared=True, passes=p))
                assert torch.equal(frows, rows)
                if r:
                    forced[p].append(tp)
        assert torch.equal(drows, rows) and torch.equal(dd2.view(torch.int32), d2.view(torch.int32))
        mm = min(m, 32)
        assert torch.equal(drows[:, :mm], srows[:, :mm])
        assert bool((lims[1:] - lims[:-1] >= found).all())
        rec = {"what": "search_deep", "n": a.n, "D": D, "K": K, "nq": a.nq, "nprobe": nprobe, "m": m,
               **{k: _stat(v) for k, v in t.items()}, "range_hits": int(lims[-1]), "found": int(found.sum()),
               "forced_passes_median_ms": {p: round(statistics.median(v), 4) for p, v in forced.items()},
               **phases(index._index, Q, km.cluster_centers_, pk, m, nprobe, min(a.repeats, 5))}
        rec["deep_over_search_32"] = round(rec["search_deep"]["median_ms"] / rec["search_32"]["median_ms"], 3)
        rec["deep_over_range"] = round(rec["search_deep"]["median_ms"] / rec["range_search"]["median_ms"], 3)
        print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
