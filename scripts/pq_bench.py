"""build_pq_index / PQIndex.search on the GPU beside build_index / ClusterIndex.search
(docs/PQ_INDEX.md has the numbers).

bf16 blobs, D = 128, K centres from a short fit, ``M`` sub-vectors.  The driver never touches the
GPU: every step is a child process of its own under its own time limit, and the first step that
fails ends the run.  A step builds both indexes over the same rows (the first one reports the
build), then measures one query count: device-event times, median (min .. max) of ``--repeats``
after a warm pass.  It reports

* ``build``   -- the PQ build split into ``lists`` (top-1 pass and partition), ``train`` (the sample's
                 residuals and the sub-space fits) and ``encode`` (the residuals' codes, list after
                 list), the whole ``ops.pq_build``, ``ops.index_build`` beside it, and both indexes' bytes
* ``search``  -- ``PQIndex.search`` and ``ClusterIndex.search`` at the same ``nq``, ``nprobe`` and ``m`` in
                 the same process: time, queries/s, the code bytes the PQ scan streams per second and
                 the PQ search's recall@m against the flat search's rows (and how often the flat search's
                 first row is among the PQ search's m)
* ``phases``  -- one block of the PQ search by phase: probes, residuals and tables, the scan kernel
                 (at every split count), the per-query sort
* ``refine``  -- per ``--shortlist``: ``PQIndex.search(refine=)`` with device rows and with host rows (up to
                 ``--host-candidates`` candidates), its recall@m against the flat search's rows, one block by
                 phase (shortlist scan, re-rank kernel, sort) and the re-rank kernel beside the torch
                 formulation ``((X[cand] - Q[:, None]) ** 2).sum(-1)``, alternating in one process

Usage: ``python scripts/pq_bench.py [--out profiles/pq_bench.md] [--n 10000000] [--k 1024] [--pq 16]
[--nq 1 1000 100000] [--nprobe 16] [--m 10] [--shortlist 32 128 256] [--repeats 5] [--step-timeout 420]``
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D = 128


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _recall(rows, exact):
    hit = (rows[:, :, None] == exact[:, None, :]) & (rows[:, :, None] >= 0)
    return float(hit.any(2).sum()) / max(1, int((exact >= 0).sum()))


def _build_phases(X, C, M, pk, train_rows, seed):
    """The PQ build by phase (one pass: it is long), then the whole build and the flat one."""
    import torch

    from mikmeans import ops
    from mikmeans.ops import pq

    n, K, dev = X.shape[0], C.shape[0], X.device

    def lists():
        labels = torch.empty(n, dtype=torch.int32, device=dev)
        pq._nearest_lists(labels, 0, lambda: [(0, X, pk)], C, None)
        return labels, ops.partition(labels, K, want_pos=True)

    (labels, (order, offsets, rpos)), t_lists = _timed(lists)

    def train():
        ids = order[pq._sample_positions(int(offsets[K]), train_rows, seed).to(dev)]
        R = pq._residuals(X[ids], labels[ids], C, X.dtype)
        return ops.pq_train(R, M, seed=seed)

    books, t_train = _timed(train)

    def encode():
        packs = pq._codebook_packs(books, X.dtype)
        codes = torch.zeros((n + 1, M), dtype=torch.uint8, device=dev)
        for a in range(0, n, ops.PQ_ENCODE_ROWS):
            b = min(n, a + ops.PQ_ENCODE_ROWS)
            R = pq._residuals(X[a:b], labels[a:b].clamp(min=0), C, X.dtype)
            codes[torch.where(rpos[a:b] >= 0, rpos[a:b], n)] = ops.pq_encode(R, books, packs=packs)
        return codes

    codes, t_encode = _timed(encode)
    del codes, labels, order, rpos
    index, t_build = _timed(lambda: ops.pq_build(X, C, M, pack=pk, train_rows=train_rows, seed=seed))
    assert torch.equal(index.codebooks, books)
    flat, t_flat = _timed(lambda: ops.index_build(X, C, pack=pk))
    return index, flat, {"lists_ms": round(t_lists, 2), "train_ms": round(t_train, 2), "encode_ms": round(t_encode, 2),
                         "pq_build_ms": round(t_build, 2), "index_build_ms": round(t_flat, 2)}


def step(a, nq: int, report_build: bool) -> int:
    import torch

    import mikmeans
    from mikmeans import ops
    from mikmeans.data import blobs as B

    if not torch.cuda.is_available():
        raise SystemExit("pq_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    K, m, M, nprobe = a.k, a.m, a.pq, a.nprobe
    X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
    km = mikmeans.KMeans(K, dtype="bfloat16", init="random", max_iter=3, seed=0).fit(X[: min(a.n, 1 << 20)])
    C = km.cluster_centers_
    pk = ops.pack_centers(C, D, X.dtype, dev)
    ops.pq_build(X[: 1 << 16], C, M, pack=pk, train_rows=4096, max_iter=2)        # (warms every code object)
    index, flat, bt = _build_phases(X, C, M, pk, a.train_rows, 0)
    if report_build:
        n = a.n
        assert index.nbytes == n * M + 8 * n + 8 * (K + 1) + 4 * M * 256 * (D // M)
        print(json.dumps({"what": "build", "n": n, "D": D, "K": K, "M": M, "train_rows": a.train_rows, **bt,
                          "pq_bytes": index.nbytes, "flat_bytes": flat.nbytes,
                          "ratio": round(flat.nbytes / index.nbytes, 2)}), flush=True)
    pqi = mikmeans.PQIndex(km, index)
    fli = mikmeans.ClusterIndex(km, flat, 0, None)
    g = torch.Generator(device="cpu").manual_seed(11)
    Q = (X[torch.randint(0, a.n, (nq,), generator=g).to(dev)].float()
         + 0.5 * torch.randn(nq, D, generator=g).to(dev)).to(torch.bfloat16)
    probes = ops.topk(Q, C, nprobe, pack=pk)[0].long()
    sizes = index.offsets[1:] - index.offsets[:-1]
    code_bytes = int(sizes[probes].sum()) * M
    pqi.search(Q, m, nprobe=nprobe)
    fli.search(Q, m, nprobe=nprobe)
    tp, tf = [], []
    for _ in range(a.repeats):
        (rows, _), t = _timed(lambda: pqi.search(Q, m, nprobe=nprobe))
        tp.append(t)
        (exact, _), t = _timed(lambda: fli.search(Q, m, nprobe=nprobe))
        tf.append(t)
    sp, sf = _stat(tp), _stat(tf)
    print(json.dumps({"what": "search", "n": a.n, "K": K, "M": M, "nq": nq, "m": m, "nprobe": nprobe, "pq": sp, "flat": sf,
                      "pq_queries_per_s": round(nq / (sp["median_ms"] / 1e3), 1),
                      "flat_queries_per_s": round(nq / (sf["median_ms"] / 1e3), 1),
                      "pq_code_gb_per_s": round(code_bytes / (sp["median_ms"] / 1e3) / 1e9, 2),
                      "recall_vs_flat": round(_recall(rows, exact), 4),
                      "flat_first_in_pq": round(float((rows == exact[:, :1]).any(1).float().mean()), 4)}), flush=True)
    # one block by phase
    nb = min(nq, ops.pq_block_queries(M, m, nprobe, D))
    Qb = Q[:nb]
    C_ = ops.require()
    cen = C.float()

    def tables():
        RQ = (Qb[:, None, :].float() - cen[probes[:nb]]).to(torch.bfloat16).view(nb * nprobe, D)
        return ops.pq_lut(RQ, index.codebooks, packs=index.packs())

    ph = {"probes": [], "tables": [], "sort": []}
    scans = {s: [] for s in (1, 2, 4, 8)}
    pr32 = probes[:nb].to(torch.int32).reshape(-1).contiguous()
    for r in range(a.repeats + 1):
        _, t0 = _timed(lambda: ops.topk(Qb, C, nprobe, pack=pk))
        lut, t1 = _timed(tables)
        ts = {}
        for s in scans:
            out = torch.empty((nb * nprobe, s, m), dtype=torch.int64, device=dev)
            _, ts[s] = _timed(lambda: C_.pq_scan(index.codes, index.order, index.offsets, lut, pr32, s, out))
        _, t3 = _timed(lambda: out.view(nb, -1).sort(dim=1).values[:, :m])
        del lut, out
        if r:
            ph["probes"].append(t0)
            ph["tables"].append(t1)
            ph["sort"].append(t3)
            for s in scans:
                scans[s].append(ts[s])
    print(json.dumps({"what": "phases", "nq": nq, "block_queries": nb, "default_splits": C_.pq_scan_splits(nb * nprobe),
                      **{k: _stat(v) for k, v in ph.items()},
                      **{f"scan_splits_{s}": _stat(v) for s, v in scans.items()},
                      "block_code_bytes": int(sizes[probes[:nb]].sum()) * M}), flush=True)
    _refined(a, nq, X, Q, C, pk, index, pqi, exact)
    return 0


def _refined(a, nq, X, Q, C, pk, index, pqi, exact):
    """``PQIndex.search(refine=)`` per shortlist, device rows and host rows: the whole search, its recall
    against the flat search's rows, one block by phase (shortlist scan with its probes and tables, the
    re-rank kernel, the sort) and the re-rank kernel beside the torch formulation
    ``((X[cand] - Q[:, None]) ** 2).sum(-1)`` on the same candidates, the two alternating."""
    import torch

    from mikmeans import ops

    m, M, nprobe, dev = a.m, a.pq, a.nprobe, X.device
    C_ = ops.require()
    Xh = None
    for S in a.shortlist:
        rec = {"what": "refine", "nq": nq, "shortlist": S, "candidates_per_query": nprobe * S}
        pqi.search(Q, m, nprobe=nprobe, refine=X, shortlist=S)
        td = []
        for _ in range(a.repeats):
            (rows, _), t = _timed(lambda: pqi.search(Q, m, nprobe=nprobe, refine=X, shortlist=S))
            td.append(t)
        rec["device_rows"] = _stat(td)
        rec["device_queries_per_s"] = round(nq / (rec["device_rows"]["median_ms"] / 1e3), 1)
        rec["recall_vs_flat"] = round(_recall(rows, exact), 4)
        rec["flat_first_in_refined"] = round(float((rows == exact[:, :1]).any(1).float().mean()), 4)
        # host rows: every block's distinct candidate rows are gathered on the host (long for many queries)
        if nq * nprobe * S <= a.host_candidates:
            if Xh is None:
                Xh = X.cpu()
            rh, _ = pqi.search(Q, m, nprobe=nprobe, refine=Xh, shortlist=S)
            assert torch.equal(rh, rows)
            th = []
            for _ in range(a.repeats):
                _, t = _timed(lambda: pqi.search(Q, m, nprobe=nprobe, refine=Xh, shortlist=S))
                th.append(t)
            rec["host_rows"] = _stat(th)
        else:
            rec["host_rows"] = "not measured"
        # one block by phase
        nb = min(nq, ops.pq_refine_block_queries(M, nprobe, D, S))
        Qb = Q[:nb].contiguous()
        ph = {"shortlist_scan": [], "rerank": [], "sort": [], "torch_formulation": []}
        for r in range(a.repeats + 1):
            cand, t0 = _timed(lambda: ops.pq_shortlist(index, Qb, C, S, nprobe, pack=pk, block_queries=nb))
            keys = torch.empty(cand.shape, dtype=torch.int64, device=dev)
            _, t1 = _timed(lambda: C_.rerank(Qb, X, cand, keys))
            _, t2 = _timed(lambda: keys.sort(dim=1).values[:, :m])
            # the torch formulation takes a [rows, R, D] temporary: in passes of at most 2^28 elements
            step_q = max(1, (1 << 28) // (cand.shape[1] * D))

            def formulation():
                cc = cand.clamp(min=0)
                return [((X[cc[s : s + step_q]] - Qb[s : s + step_q, None]) ** 2).sum(-1) for s in range(0, nb, step_q)]

            _, t3 = _timed(formulation)
            del cand, keys
            if r:
                for k, t in zip(ph, (t0, t1, t2, t3)):
                    ph[k].append(t)
        rec.update({"block_queries": nb, **{k: _stat(v) for k, v in ph.items()},
                    "rerank_row_gb_per_s": round(nb * nprobe * S * D * 2 / (statistics.median(ph["rerank"]) / 1e3) / 1e9, 1)})
        print(json.dumps(rec), flush=True)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/pq_bench.md")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--pq", type=int, default=16, metavar="M")
    ap.add_argument("--train-rows", type=int, default=65536)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 1000, 100000])
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--shortlist", type=int, nargs="*", default=[32, 128, 256], help="refined searches to measure")
    ap.add_argument("--host-candidates", type=int, default=1 << 24,
                    help="host rows are measured up to this many candidates (nq * nprobe * shortlist)")
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds one step (one query count) may take")
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)   # (a child: this query count)
    ap.add_argument("--report-build", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.step is not None:
        return step(a, a.step, a.report_build)
    recs = []
    base = [sys.executable, os.path.abspath(__file__), "--n", str(a.n), "--k", str(a.k), "--pq", str(a.pq), "--train-rows",
            str(a.train_rows), "--nprobe", str(a.nprobe), "--m", str(a.m), "--repeats", str(a.repeats),
            "--host-candidates", str(a.host_candidates), "--shortlist", *map(str, a.shortlist)]
    for i, nq in enumerate(a.nq):
        cmd = ["timeout", "-k", "10", str(a.step_timeout), *base, "--step", str(nq), *(["--report-build"] if i == 0 else [])]
        r = subprocess.run(cmd, capture_output=True, text=True)
        for line in r.stdout.splitlines():
            if line.startswith("{"):
                recs.append(json.loads(line))
                print(line, flush=True)
        if r.returncode != 0:          # a fault, an abort or the time limit: nothing more is started
            print(f"step nq={nq} ended with status {r.returncode}:\n{r.stderr[-3000:]}", file=sys.stderr, flush=True)
            return 1
    lines = [f"# build_pq_index / search beside build_index / search (bf16 blobs N={a.n} D={D} K={a.k}, M={a.pq}, "
             f"nprobe={a.nprobe}, m={a.m})", "", "```"] + [json.dumps(r) for r in recs] + ["```"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
