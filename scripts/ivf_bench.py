"""build_index / search on the GPU: the build by phase, the search at several probe counts with its
recall, a PyTorch brute force on the same queries and, at a smaller N, the exact search beside
``ops.topk`` on the same pairs (profiles/r8_01_ivf.md).

One process, device-event times taken after a warm pass.  bf16 blobs, D = 128, K centres from a
short fit.  It reports

* ``build``   -- ``lists`` (the top-1 pass over the row blocks and each row's list), ``partition``
                 (csrc/ivf.hip count / scan / scatter), ``pack`` (the row pack, its buffers filled
                 first) and the whole ``ops.index_build``
* ``search``  -- ``ops.index_search`` for nq queries at each nprobe: time, queries/s and recall@m
                 against the index's own nprobe = K answer (the exact search over the indexed rows)
* ``brute``   -- blocked ``Q @ X.T`` + ``torch.topk`` in PyTorch on the same rows and queries
* ``exact``   -- at ``--n-exact`` rows: ``index_search(nprobe=K)`` beside ``ops.topk(Q, X.float(), m)``,
                 the top-m kernel with the rows packed as centres (the same pairs, no lists)

Usage: ``python scripts/ivf_bench.py [--out profiles/r8_01_ivf.md] [--n 10000000] [--k 1024]
[--nq 10000 1] [--nprobe 1 4 16 64] [--m 10] [--repeats 5]``
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


def _lists(X, C, pk):
    labels = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    for s, idx, d2 in ops.topk_blocks(X, C, 1, pack=pk):
        labels[s : s + idx.shape[0]] = torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1)
    return labels


def _pack(X, K, labels, rpos, offsets):
    n = X.shape[0]
    toff = torch.zeros(K + 1, dtype=torch.int64, device=X.device)
    toff[1:] = torch.cumsum((offsets[1:] - offsets[:-1] + 15) // 16, 0)
    tiles = ops.index_tiles(n, K)
    pack = torch.zeros(tiles * 16 * D, dtype=X.dtype, device=X.device)
    cn = torch.full((tiles * 16,), 1e30, dtype=torch.float32, device=X.device)
    ops.require().ivf_pack(X, 0, labels, rpos, offsets, toff, pack, cn, D)
    return pack, cn


def build_phases(X, C, pk, repeats):
    K = C.shape[0]
    t = {k: [] for k in ("lists", "partition", "pack", "build")}
    for r in range(repeats + 1):                              # (the first pass warms every code object)
        labels, a = _timed(lambda: _lists(X, C, pk))
        (order, offsets, rpos), b = _timed(lambda: ops.partition(labels, K, want_pos=True))
        packed, c = _timed(lambda: _pack(X, K, labels, rpos, offsets))
        del packed
        index, d = _timed(lambda: ops.index_build(X, C, pack=pk))
        if r:
            for k, v in zip(t, (a, b, c, d)):
                t[k].append(v)
        if r < repeats:
            del index
    return index, {k: _stat(v) for k, v in t.items()}


def brute_force(X, xn, Q, m, block=1 << 17):
    """PyTorch: |x|^2 - 2 q.x per row block (bf16 GEMM, f32 scores), torch.topk, a running merge."""
    best = torch.full((Q.shape[0], m), float("inf"), device=Q.device)
    rows = torch.full((Q.shape[0], m), -1, dtype=torch.int64, device=Q.device)
    for s in range(0, X.shape[0], block):
        sc = xn[None, s : s + block] - 2.0 * (Q @ X[s : s + block].T).float()
        v, i = torch.topk(sc, min(m, sc.shape[1]), dim=1, largest=False)
        v, o = torch.topk(torch.cat([best, v], 1), m, dim=1, largest=False)
        rows = torch.cat([rows, i + s], 1).gather(1, o)
        best = v
    return rows, best


def _recall(rows, exact):
    hit = (rows[:, :, None] == exact[:, None, :]) & (rows[:, :, None] >= 0)
    return float(hit.any(2).sum()) / max(1, int((exact >= 0).sum()))


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r8_01_ivf.md")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--n-exact", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--nq", type=int, nargs="+", default=[10_000, 1])
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 4, 16, 64])
    ap.add_argument("--m", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ivf_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    K, m = a.k, a.m
    X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
    km = mikmeans.KMeans(K, dtype="bfloat16", init="random", max_iter=3, seed=0).fit(X[: min(a.n, 1 << 20)])
    C = km.cluster_centers_
    pk = ops.pack_centers(C, D, X.dtype, dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    recs = []
    head = f"# build_index / search: build by phase, search by nprobe, brute force (bf16 blobs N={a.n} D={D} K={K}, m={m})"
    lines = [head, "",
             f"`python scripts/ivf_bench.py --n {a.n} --n-exact {a.n_exact} --k {K} --nq {' '.join(map(str, a.nq))} "
             f"--nprobe {' '.join(map(str, a.nprobe))} --m {m} --repeats {a.repeats}` on {torch.cuda.get_device_name(0)}: "
             f"device-event times in ms, median (min .. max) of {a.repeats} repeats after a warm pass.", ""]

    def cell(s):
        return f"{s['median_ms']:.3f} ({s['min_ms']:.3f} .. {s['max_ms']:.3f})"

    index, bt = build_phases(X, C, pk, a.repeats)
    sizes = (index.offsets[1:] - index.offsets[:-1]).float()
    rec = {"what": "build", "n": a.n, "D": D, "K": K, **bt, "index_bytes": index.nbytes,
           "list_rows_mean": round(float(sizes.mean()), 1), "list_rows_max": int(sizes.max())}
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    lines += ["| build phase | ms |", "|---|---|"] + [f"| {k} | {cell(v)} |" for k, v in bt.items()]
    lines += ["", f"Index: {index.nbytes / 1e9:.3f} GB; lists of {rec['list_rows_mean']} rows on average, "
                  f"{rec['list_rows_max']} the longest.", "",
              "| nq | nprobe | search ms | queries/s | recall@m | brute force ms |", "|---|---|---|---|---|---|"]
    xn = ops.row_sqnorm(X)
    for nq in a.nq:
        Q = (X[torch.randint(0, a.n, (nq,), generator=g).to(dev)].float()
             + 0.5 * torch.randn(nq, D, generator=g).to(dev)).to(torch.bfloat16)
        exact = ops.index_decode(ops.index_search(index, Q, C, m, K, pack=pk))[0]
        brute_force(X, xn, Q, m)
        tb = [_timed(lambda: brute_force(X, xn, Q, m))[1] for _ in range(a.repeats)]
        for nprobe in [*a.nprobe, K]:
            ops.index_search(index, Q, C, m, nprobe, pack=pk)
            outs = [_timed(lambda: ops.index_search(index, Q, C, m, nprobe, pack=pk)) for _ in range(a.repeats)]
            st = _stat([t for _, t in outs])
            rows = ops.index_decode(outs[-1][0])[0]
            rec = {"what": "search", "n": a.n, "K": K, "nq": nq, "m": m, "nprobe": nprobe, **st,
                   "queries_per_s": round(nq / (st["median_ms"] / 1e3), 1), "recall": round(_recall(rows, exact), 4),
                   "brute": _stat(tb)}
            recs.append(rec)
            print(json.dumps(rec), flush=True)
            lines.append(f"| {nq} | {nprobe} | {cell(st)} | {rec['queries_per_s']:.0f} | {rec['recall']:.4f} | "
                         f"{cell(rec['brute'])} |")
    del index, xn
    # the exact search beside the top-m kernel on the same pairs
    Xe = X[: a.n_exact]
    nq = a.nq[0]
    Q = (Xe[torch.randint(0, a.n_exact, (nq,), generator=g).to(dev)].float()
         + 0.5 * torch.randn(nq, D, generator=g).to(dev)).to(torch.bfloat16)
    index = ops.index_build(Xe, C, pack=pk)
    rp = ops.pack_centers(Xe.float(), D, Xe.dtype, dev)
    Xf = Xe.float()
    t = {"search_nprobe_K": [], "topk_rows_as_centres": []}
    for r in range(a.repeats + 1):
        keys, ts = _timed(lambda: ops.index_search(index, Q, C, m, K, pack=pk))
        (ti, td), tt = _timed(lambda: ops.topk(Q, Xf, m, pack=rp))
        if r:
            t["search_nprobe_K"].append(ts)
            t["topk_rows_as_centres"].append(tt)
    rows, d2 = ops.index_decode(keys)
    assert torch.equal(rows, ti.long()) and torch.equal(d2, td)          # the same pairs, the same answer
    st = {k: _stat(v) for k, v in t.items()}
    rec = {"what": "exact", "n": a.n_exact, "K": K, "nq": nq, "m": m, **st,
           "ratio": round(st["search_nprobe_K"]["median_ms"] / st["topk_rows_as_centres"]["median_ms"], 4)}
    recs.append(rec)
    print(json.dumps(rec), flush=True)
    lines += ["", f"Exact search at N = {a.n_exact}, nq = {nq}: `index_search(nprobe=K)` {cell(st['search_nprobe_K'])} ms, "
                  f"`ops.topk(Q, X.float(), {m})` on the packed rows {cell(st['topk_rows_as_centres'])} ms "
                  f"(ratio {rec['ratio']:.3f}); the two answers are bitwise equal."]
    lines += ["", "```"] + [json.dumps(r) for r in recs] + ["```"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
