"""cluster_quantiles on the GPU: every histogram pass in both of the kernel's forms and with and
without wave aggregation, the selects, the four passes together, the whole call, the top-1 pass it
rides on, and the sort it replaces (profiles/r7_03_quantiles.md).

One process, the arms interleaved inside every repeat, device-event times taken after two warm
passes, the GFX clock sampled over the timed repeats (mikmeans/utils/telemetry.py).  bf16
blobs, D = 128, rows in blocks of 2^22 as ``ops.quantile_top1`` takes them.  Per (K, Q):

* ``top1``     -- ``ops.topk(X, C, 1)`` over the row blocks: the pass the call makes once
* ``sort``     -- the baseline: a stable ``torch.sort`` of the ``label << 32 | bits`` int64 keys of
                  the same rows (``keys``: building them from the top-1 output)
* ``p0``..``p3`` -- ``ops.quantile_hist`` of one pass on the kept top-1 output, the prefixes
                  those of the real select: ``g`` the global form, ``l`` the LDS-private one
                  (where the lists fit), each with ``agg`` rounds of wave aggregation, ``b`` the
                  banded LDS form (more lists than one workgroup holds); then the same with the rows
                  ordered by label (``o0``..``o3``), which puts every wave on one cluster
* ``selects``  -- the four ``ops.quantile_select`` launches
* ``passes``   -- ``ops.quantile_passes`` whole: four histograms by the launcher's rule, the
                  selects, the tables' zeroing and the decode
* ``call``     -- ``ops.cluster_quantiles`` whole (top-1 passes and ``passes``), on packed centres

With ``--small-n`` the first (K, Q) rows with K <= 160 also time passes 0 and 1 on few rows, one
launch, in the global and the LDS form: the row count from which the LDS form pays.

Every arm of a pass must give the same table, and the passes the values read off the sorted keys.

Usage: ``python scripts/quantiles_bench.py [--out profiles/r7_03_quantiles.md] [--n 10000000]
[--k 8 160 1024 4096] [--q 1 3 8] [--agg 0 4] [--small-n ...] [--repeats 5]``
"""
from __future__ import annotations

import argparse
import collections
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mikmeans import ops  # noqa: E402
from mikmeans.data import blobs as B  # noqa: E402

D = 128
BLOCK = ops.QUANTILE_BLOCK_ROWS
LEVELS = {1: (0.5,), 3: (0.5, 0.9, 0.99), 8: (0.0, 0.05, 0.1, 0.25, 0.5, 0.9, 0.99, 1.0)}


def _events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return out, (e0, e1)


def _ms(pairs):
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs)


def top1(X, C, pk):
    """The top-1 output of every row block and the pass's time."""
    outs, evs = [], []
    for s in range(0, X.shape[0], BLOCK):
        o, ev = _events(lambda: ops.topk(X[s : s + BLOCK], C, 1, pack=pk))
        outs.append(o)
        evs.append(ev)
    return outs, _ms(evs)


def hist(chunks, K, prefix, p, path, agg):
    """One pass's table and the time of its launches (the table zeroed outside the window)."""
    shape = (K, ops.QUANTILE_BINS) if p == 0 else (K, prefix.shape[1], ops.QUANTILE_BINS)
    table = torch.zeros(shape, dtype=torch.int64, device=prefix.device)
    evs = []
    for idx, d2 in chunks:
        _, ev = _events(lambda: ops.quantile_hist(idx, d2, K, prefix, p, table=table, path=path, agg=agg))
        evs.append(ev)
    return table, _ms(evs)


def select_chain(chunks, K, qt):
    """The real select: (prefix before each pass, the tables, the time of the four selects)."""
    prefix, rank, counts = ops.quantile_state(K, qt.shape[0], qt.device)
    before, tables, evs = [], [], []
    for p in range(ops.QUANTILE_PASSES):
        before.append(prefix.clone())
        table, _ = hist(chunks, K, prefix, p, -1, -1)
        tables.append(table)
        _, ev = _events(lambda: ops.quantile_select(table, qt, prefix, rank, counts, p))
        evs.append(ev)
    return before, tables, _ms(evs), prefix, counts


def sort_baseline(chunks):
    def key(i, d):
        return (i[:, 0].to(torch.int64) << 32) | (d[:, 0].clamp_min(0.0) + 0.0).view(torch.int32).to(torch.int64)

    (keys, ev_k) = _events(lambda: torch.cat([key(i, d) for i, d in chunks]))
    t_keys = _ms([ev_k])
    (out, ev_s) = _events(lambda: torch.sort(keys, stable=True).values)
    return out, t_keys, _ms([ev_s])


def from_sorted(keys, K, qs):
    """The quantiles read off the sorted keys (blobs: every label in range, every distance finite
    and positive): squared-distance bits int64 [K, Q], -1 for a cluster without rows."""
    lab = keys >> 32
    n = torch.bincount(lab, minlength=K)
    first = torch.cumsum(n, 0) - n
    q = torch.tensor(qs, dtype=torch.float64, device=keys.device)
    r = torch.ceil(q[None, :] * n.to(torch.float64)[:, None]).to(torch.int64) - 1
    r = torch.minimum(r, n[:, None] - 1).clamp_min(0)
    pos = (first[:, None] + r).clamp_max(keys.shape[0] - 1)
    return torch.where(n[:, None] > 0, keys[pos] & 0xFFFFFFFF, -1)


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r7_03_quantiles.md")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, nargs="+", default=[8, 160, 1024, 4096])
    ap.add_argument("--q", type=int, nargs="+", default=[1, 3, 8], choices=sorted(LEVELS))
    ap.add_argument("--agg", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--small-n", type=int, nargs="*", default=[1024, 4096, 8192, 16384, 65536, 262144])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("quantiles_bench.py measures on the GPU; none found")
    from mikmeans.utils.telemetry import ClockSampler

    dev = torch.device("cuda")
    C_ = ops.require()
    arms = [(path, agg) for path in (0, 1) for agg in a.agg] + [(2, 0)]
    head = (f"# cluster_quantiles: histogram passes (global / LDS form, wave aggregation), selects, whole call, "
            f"top-1 pass and the sort baseline (bf16 blobs N={a.n} D={D})")
    lines = [head, "",
             f"`python scripts/quantiles_bench.py --n {a.n} --k {' '.join(map(str, a.k))} --q {' '.join(map(str, a.q))} "
             f"--agg {' '.join(map(str, a.agg))} --repeats {a.repeats}` on {torch.cuda.get_device_name(0)}: device-event "
             f"times in ms, median (min .. max) of {a.repeats} interleaved repeats after two warm passes; row blocks of "
             f"{BLOCK}; the built aggregation depths are {C_.QUANTILE_AGG_ROUNDS} (global form) and "
             f"{C_.QUANTILE_LDS_AGG_ROUNDS} (LDS form).", "",
             "| K | Q | top1 | sort (keys) | selects | passes | call | passes / sort | clock MHz |",
             "|---|---|---|---|---|---|---|---|---|"]
    plines = ["", "Histogram passes, median ms: `g` global form, `l` LDS form, `b` banded LDS form, `@a` rounds of wave "
              "aggregation; `-` where the form does not take the lists; bold the fastest of the pass.", "",
              "| K | Q | pass | " + " | ".join(f"{'glb'[p]}@{g}" for p, g in arms) + " | rule takes |",
              "|---|---|---|" + "---|" * (len(arms) + 1)]
    slines = ["", f"Few rows, one launch, Q = {a.q[0]}, each form with its built aggregation depth: median (min .. max) of "
              f"{4 * a.repeats} alternating repeats.", "",
              "| K | rows | pass 0 global | pass 0 lds (K > 160: banded) | pass 1 global | pass 1 lds (banded) |", "|---|---|---|---|---|---|"]
    recs = []
    for K in a.k:
        X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
        C = B.blob_centers(K, D, 10.0, 7, device=dev)
        pk = ops.pack_centers(C, D, X.dtype, dev)
        for Q in a.q:
            qs = LEVELS[Q]
            qt = torch.tensor(qs, dtype=torch.float64, device=dev)

            def fits(p, path=1):
                lists, held = (K if p == 0 else K * Q), C_.QUANTILE_LDS_MAX_LISTS
                return lists <= held if path == 1 else held < lists <= held * C_.QUANTILE_BAND_LIMIT

            def one_repeat(r, t):
                chunks, tt = top1(X, C, pk)
                t["top1"].append(tt)
                keys, tk, ts = sort_baseline(chunks)
                t["keys"].append(tk)
                t["sort"].append(ts)
                before, tables, tsel, _, _ = select_chain(chunks, K, qt)
                t["selects"].append(tsel)
                for p in range(ops.QUANTILE_PASSES):
                    order = [(path, agg) for path, agg in arms if path == 0 or fits(p, path)]
                    for path, agg in (order if r % 2 == 0 else order[::-1]):
                        table, th = hist(chunks, K, before[p], p, path, agg)
                        assert torch.equal(table, tables[p]), (K, Q, p, path, agg)      # the arms computed the same thing
                        t[f"p{p}_{'glb'[path]}{agg}"].append(th)
                # the same rows ordered by label: every wave on one cluster, all waves in step
                by_label = []
                for i, d in chunks:
                    o = torch.argsort(i[:, 0], stable=True)
                    by_label.append((i[o].contiguous(), d[o].contiguous()))
                for p in range(ops.QUANTILE_PASSES):
                    order = [(path, agg) for path, agg in arms if path == 0 or fits(p, path)]
                    for path, agg in (order if r % 2 == 0 else order[::-1]):
                        table, th = hist(by_label, K, before[p], p, path, agg)
                        assert torch.equal(table, tables[p]), (K, Q, p, path, agg, "by label")
                        t[f"o{p}_{'glb'[path]}{agg}"].append(th)
                del by_label
                (out, ev) = _events(lambda: ops.quantile_passes(chunks, K, qs, dev))
                t["passes"].append(_ms([ev]))
                (whole, ev) = _events(lambda: ops.cluster_quantiles(X, C, qs, pack=pk))
                t["call"].append(_ms([ev]))
                exp = from_sorted(keys, K, qs)
                for v, n in (out, whole):
                    got = torch.where((n > 0)[:, None], v.view(torch.int32).to(torch.int64), -1)
                    assert torch.equal(got, exp), (K, Q)
                del keys

            for r in range(2):                                      # warm every shape and code object
                one_repeat(r, collections.defaultdict(list))
            t = collections.defaultdict(list)
            with ClockSampler(0, period_s=0.02) as cs:
                for r in range(a.repeats):
                    one_repeat(r, t)
            sm = cs.summary() or {}
            st = {k: _stat(v) for k, v in t.items()}
            rule = {p: int(C_.quantile_path(min(a.n, BLOCK), K if p == 0 else K * Q, p)) for p in range(4)}
            rec = {"n": a.n, "D": D, "K": K, "Q": Q, "q": list(qs), "dtype": "bfloat16",
                   "rule_path": [rule[p] for p in range(4)], "agg_built": int(C_.QUANTILE_AGG_ROUNDS),
                   "agg_lds_built": int(C_.QUANTILE_LDS_AGG_ROUNDS), **st,
                   "passes_over_sort": round(st["passes"]["median_ms"] / st["sort"]["median_ms"], 4),
                   "passes_share_of_call": round(st["passes"]["median_ms"] / st["call"]["median_ms"], 4),
                   "clock_mhz": sm.get("clock_mhz")}
            recs.append(rec)
            print(json.dumps(rec), flush=True)

            def cell(k):
                return f"{st[k]['median_ms']:.3f} ({st[k]['min_ms']:.3f} .. {st[k]['max_ms']:.3f})" if k in st else "-"

            lines.append(f"| {K} | {Q} | {cell('top1')} | {cell('sort')} ({st['keys']['median_ms']:.3f}) | {cell('selects')} | "
                         f"{cell('passes')} | {cell('call')} | {rec['passes_over_sort']:.2f} | "
                         f"{rec['clock_mhz'] or 'not read'} |")
            for tag, label in (("p", ""), ("o", " by label")):
                for p in range(4):
                    names = [f"{tag}{p}_{'glb'[path]}{agg}" for path, agg in arms]
                    best = min((st[nm]["median_ms"] for nm in names if nm in st))
                    cells = [("-" if nm not in st else
                              (f"**{st[nm]['median_ms']:.3f}**" if st[nm]["median_ms"] == best
                               else f"{st[nm]['median_ms']:.3f}")) for nm in names]
                    plines.append(f"| {K} | {Q} | {p}{label} | " + " | ".join(cells) +
                                  f" | {('global', 'lds', 'banded')[rule[p]]} |")
            if Q == a.q[0] and K * Q <= C_.QUANTILE_LDS_MAX_LISTS * C_.QUANTILE_BAND_LIMIT and a.small_n:
                # the row count from which the LDS form (K <= 160; the banded one past it) pays: one
                # launch, passes 0 and 1, Q as above
                lds = 1 if K * Q <= C_.QUANTILE_LDS_MAX_LISTS else 2
                chunks, _ = top1(X[: max(a.small_n)], C, pk)
                before = select_chain(chunks, K, qt)[0]
                for n in a.small_n:
                    part = [(chunks[0][0][:n], chunks[0][1][:n])]
                    ts = collections.defaultdict(list)
                    for r in range(2 + 4 * a.repeats):
                        for p in (0, 1):
                            for path in ((0, lds) if r % 2 == 0 else (lds, 0)):
                                _, th = hist(part, K, before[p], p, path, -1)
                                if r >= 2:
                                    ts[f"p{p}_{'gl'[path > 0]}"].append(th)
                    srec = {"small_n": n, "K": K, "Q": Q, **{k: _stat(v) for k, v in ts.items()}}
                    recs.append(srec)
                    print(json.dumps(srec), flush=True)
                    slines.append(f"| {K} | {n} | " + " | ".join(
                        f"{srec[k]['median_ms']:.4f} ({srec[k]['min_ms']:.4f} .. {srec[k]['max_ms']:.4f})"
                        for k in ("p0_g", "p0_l", "p1_g", "p1_l")) + " |")
        del X
    lines += plines + (slines if len(slines) > 5 else []) + ["", "```"] + [json.dumps(r) for r in recs] + ["```"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
