"""cluster_exemplars on the GPU: the accumulate kernel in both of its forms, the whole call and
the top-1 pass it rides on (profiles/r7_02_exemplars.md).

One process, the arms interleaved inside every repeat, device-event times taken after two warm
passes, the GFX clock sampled over the timed repeats (mikmeans/utils/telemetry.py).  bf16
blobs, D = 128, rows in blocks of 2^22 as ``ops.exemplar_rows`` takes them.  Per (K, m, mode):

* ``top1``    -- ``ops.topk(X, C, 1)`` over the row blocks: the pass every arm shares (it exists
                 without this kernel and is the yardstick)
* ``global``  -- ``ops.exemplar_accumulate(path=0)`` on the top-1 output: rows straight into the
                 global table
* ``lds``     -- the same with ``path=1``: a private table per workgroup in LDS, then the flush
* ``call``    -- ``ops.cluster_exemplars`` whole (top-1 passes, accumulate by the launcher's rule,
                 decode), on packed centres

The two forms must give the same table, and the whole call the lists decoded from it.

Usage: ``python scripts/exemplars_bench.py [--out profiles/r7_02_exemplars.md] [--n 10000000]
[--k 1024] [--m 1 8 32] [--repeats 7]``
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mikmeans import ops  # noqa: E402
from mikmeans.data import blobs as B  # noqa: E402

D = 128
BLOCK = ops.EXEMPLAR_BLOCK_ROWS


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


def accumulate(blocks, K, m, far, path):
    table = ops.exemplar_new(K, m, blocks[0][0].device)
    evs, s = [], 0
    for idx, d2 in blocks:
        _, ev = _events(lambda: ops.exemplar_accumulate(table, idx, d2, row0=s, farthest=far, path=path))
        evs.append(ev)
        s += idx.shape[0]
    return table, _ms(evs)


def whole(X, C, pk, m, far):
    out, ev = _events(lambda: ops.cluster_exemplars(X, C, m, farthest=far, pack=pk))
    return out, _ms([ev])


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r7_02_exemplars.md")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, nargs="+", default=[1024])
    ap.add_argument("--m", type=int, nargs="+", default=[1, 8, 32])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("exemplars_bench.py measures on the GPU; none found")
    from mikmeans.utils.telemetry import ClockSampler

    dev = torch.device("cuda")
    C_ = ops.require()
    head = (f"# cluster_exemplars: accumulate kernel (global / LDS form), whole call and top-1 pass "
            f"(bf16 blobs N={a.n} D={D})")
    lines = [head, "",
             f"`python scripts/exemplars_bench.py --n {a.n} --k {' '.join(map(str, a.k))} --m {' '.join(map(str, a.m))} "
             f"--repeats {a.repeats}` on {torch.cuda.get_device_name(0)}: device-event times in ms, median (min .. max) "
             f"of {a.repeats} interleaved repeats after two warm passes; row blocks of {BLOCK}.", "",
             "| K | m | mode | top1 | global | lds | rule takes | call | accumulate share of call | clock MHz |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    recs = []
    for K in a.k:
        X = B.make_blobs(a.n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
        C = B.blob_centers(K, D, 10.0, 7, device=dev)
        pk = ops.pack_centers(C, D, X.dtype, dev)
        for m in a.m:
            fits = K * m <= C_.EXEMPLAR_LDS_MAX_WORDS
            for far in (False, True):
                paths = [0, 1] if fits else [0]
                for _ in range(2):                                  # warm every shape and code object
                    blocks, _t = top1(X, C, pk)
                    for p in paths:
                        accumulate(blocks, K, m, far, p)
                    whole(X, C, pk, m, far)
                t = {k: [] for k in ("top1", "global", "lds", "call")}
                with ClockSampler(0, period_s=0.02) as cs:
                    for r in range(a.repeats):
                        blocks, tt = top1(X, C, pk)
                        t["top1"].append(tt)
                        tabs = {}
                        for p in (paths if r % 2 == 0 else paths[::-1]):
                            tabs[p], ta = accumulate(blocks, K, m, far, p)
                            t["global" if p == 0 else "lds"].append(ta)
                        (rows, d2, table), tc = whole(X, C, pk, m, far)
                        t["call"].append(tc)
                sm = cs.summary() or {}
                # the arms computed the same thing
                assert all(torch.equal(tabs[p], table) for p in paths)
                er, ed = ops.exemplar_decode(table, farthest=far)
                assert torch.equal(er, rows) and torch.equal(ed.view(torch.int32), d2.view(torch.int32))
                st = {k: _stat(v) for k, v in t.items() if v}
                uses_lds = bool(C_.exemplar_uses_lds(min(a.n, BLOCK), K, m))
                rule = st["lds" if uses_lds else "global"]["median_ms"]
                rec = {"n": a.n, "D": D, "K": K, "m": m, "farthest": far, "dtype": "bfloat16", "rule_uses_lds": uses_lds,
                       **st, "accumulate_share_of_call": round(rule / st["call"]["median_ms"], 4),
                       "clock_mhz": sm.get("clock_mhz")}
                recs.append(rec)
                print(json.dumps(rec), flush=True)

                def cell(k):
                    return f"{st[k]['median_ms']:.3f} ({st[k]['min_ms']:.3f} .. {st[k]['max_ms']:.3f})" if k in st else "-"

                lines.append(f"| {K} | {m} | {'farthest' if far else 'nearest'} | {cell('top1')} | {cell('global')} | "
                             f"{cell('lds')} | {'lds' if uses_lds else 'global'} | {cell('call')} | "
                             f"{100 * rec['accumulate_share_of_call']:.1f} % | {rec['clock_mhz'] or 'not read'} |")
        del X
    lines += ["", "```"] + [json.dumps(r) for r in recs] + ["```"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
