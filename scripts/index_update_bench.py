"""ClusterIndex add / remove / save / load on the GPU beside the full build (docs/INDEX_UPDATES.md).

One process, device-event times taken after a warm pass, median (min .. max) of ``--repeats`` runs.
bf16 blobs, D = 128, K centres from a short fit.  It reports

* ``build``   -- ``ops.index_build`` over all N rows
* ``add``     -- for each ``--frac`` of N new rows on top of the N: ``ops.index_add`` whole, and its
                 phases on the same tensors: ``top1`` (the new rows' lists), ``order`` (every id's
                 list and position from the old index, the partition, the tile offsets), ``fill``
                 (the new buffers, zeros and PAD_SCORE), ``repack`` (csrc/ivf.hip: the old rows
                 from the old pack into the new one) and ``pack`` (the new rows through the row pack)
* ``remove``  -- for each ``--frac`` of the N ids, drawn at random: ``ops.index_remove`` whole and
                 its ``repack``
* ``save`` / ``load`` -- ``ClusterIndex.save`` to ``--dir`` and ``ClusterIndex.load`` back (wall clock)

The repack's rate counts the bytes of the rows it moves, read from the old pack and written to the
new one (rows and cn); ``scripts/hbm_ceiling.py`` gives the box's copy / fill rates to set it beside.

Usage: ``python scripts/index_update_bench.py [--out profiles/r10_01_index_updates.md] [--json FILE]
[--n 10000000] [--k 1024] [--frac 0.01 0.1] [--repeats 5] [--dir DIR]``
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import mikmeans  # noqa: E402
from mikmeans import ops  # noqa: E402
from mikmeans.data import blobs as B  # noqa: E402
from mikmeans.ops import index as I  # noqa: E402

D = 128


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1)


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _lists(X, C, pk):
    labels = torch.empty(X.shape[0], dtype=torch.int32, device=X.device)
    for s, idx, d2 in ops.topk_blocks(X, C, 1, pack=pk):
        labels[s : s + idx.shape[0]] = torch.where(torch.isfinite(d2[:, 0]), idx[:, 0], -1)
    return labels


def _order(index, new_labels, gone=None):
    """Every id's list and position in the old index, the new partition and the tile offsets."""
    lab_old, rpos_old = I._id_lists(index)
    if gone is not None:
        lab_old = torch.where(gone, -1, lab_old)
    labels = lab_old if new_labels is None else torch.cat([lab_old, new_labels])
    order, offsets, rpos = ops.partition(labels, index.K, want_pos=True)
    toff = torch.zeros(index.K + 1, dtype=torch.int64, device=labels.device)
    toff[1:] = torch.cumsum((offsets[1:] - offsets[:-1] + 15) // 16, 0)
    return labels, rpos_old, order, offsets, rpos, toff


def _fill(index, n):
    tiles = ops.index_tiles(n, index.K)
    pack = torch.zeros(tiles * 16 * index.cols, dtype=index.dtype, device=index.pack.device)
    cn = torch.full((tiles * 16,), 1e30, dtype=torch.float32, device=index.pack.device)
    return pack, cn


def _repack(index, rpos_old, order, offsets, toff, pack, cn):
    ops.require().ivf_repack(index.pack, index.cn, index.offsets, index.tile_offsets, rpos_old, order, offsets, toff,
                             pack, cn, index.D, index.cols)


def _moved_bytes(index, rows):
    """Bytes the repack reads and writes for ``rows`` rows: each row and its cn, once in, once out."""
    return 2 * rows * (index.cols * index.pack.element_size() + 4)


def add_phases(index, X1, C, pk, repeats):
    t = {k: [] for k in ("top1", "order", "fill", "repack", "pack", "add")}
    n0 = index.n
    for r in range(repeats + 1):                              # (the first pass warms every code object)
        new_labels, a = _timed(lambda: _lists(X1, C, pk))
        (labels, rpos_old, order, offsets, rpos, toff), b = _timed(lambda: _order(index, new_labels))
        (pack, cn), c = _timed(lambda: _fill(index, labels.numel()))
        _, d = _timed(lambda: _repack(index, rpos_old, order, offsets, toff, pack, cn))
        _, e = _timed(lambda: ops.require().ivf_pack(X1, n0, labels, rpos, offsets, toff, pack, cn, index.cols))
        del pack, cn, labels, rpos_old, order, offsets, rpos, toff
        new, f = _timed(lambda: ops.index_add(index, X1, C, pack=pk))
        del new
        if r:
            for k, v in zip(t, (a, b, c, d, e, f)):
                t[k].append(v)
    return {k: _stat(v) for k, v in t.items()}


def remove_phases(index, ids, repeats):
    t = {k: [] for k in ("order", "fill", "repack", "remove")}
    gone = torch.zeros(index.n, dtype=torch.bool, device=ids.device)
    gone[ids] = True
    for r in range(repeats + 1):
        (labels, rpos_old, order, offsets, rpos, toff), b = _timed(lambda: _order(index, None, gone))
        (pack, cn), c = _timed(lambda: _fill(index, index.n))
        _, d = _timed(lambda: _repack(index, rpos_old, order, offsets, toff, pack, cn))
        del pack, cn, labels, rpos_old, order, offsets, rpos, toff
        (new, removed), f = _timed(lambda: ops.index_remove(index, ids))
        del new
        if r:
            for k, v in zip(t, (b, c, d, f)):
                t[k].append(v)
    return {k: _stat(v) for k, v in t.items()}, int(removed)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/r10_01_index_updates.md")
    ap.add_argument("--json", default=None, help="also write the one JSON record here")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--frac", type=float, nargs="+", default=[0.01, 0.1])
    ap.add_argument("--dir", default=None, help="where save / load go (default: a temporary directory)")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("index_update_bench.py measures on the GPU; none found")
    dev = torch.device("cuda")
    K, n = a.k, a.n
    extra = max(int(round(f * n)) for f in a.frac)
    X = B.make_blobs(n + extra, D, K, seed=7, dtype=torch.bfloat16, device=dev)
    km = mikmeans.KMeans(K, dtype="bfloat16", init="random", max_iter=3, seed=0).fit(X[: min(n, 1 << 20)])
    C = km.cluster_centers_
    pk = ops.pack_centers(C, D, X.dtype, dev)
    g = torch.Generator(device="cpu").manual_seed(11)
    rec = {"what": "index_updates", "device": torch.cuda.get_device_name(0), "n": n, "D": D, "K": K,
           "repeats": a.repeats}

    def cell(s):
        return f"{s['median_ms']:.3f} ({s['min_ms']:.3f} .. {s['max_ms']:.3f})"

    tb = []
    for r in range(a.repeats + 1):
        index, t = _timed(lambda: ops.index_build(X[:n], C, pack=pk))
        if r:
            tb.append(t)
        if r < a.repeats:
            del index
    rec["build"] = _stat(tb)
    rec["index_bytes"] = index.nbytes
    print(json.dumps({"build": rec["build"]}), flush=True)
    lines = [f"# ClusterIndex updates beside the build (bf16 blobs N={n} D={D} K={K})", "",
             f"`python scripts/index_update_bench.py --n {n} --k {K} --frac {' '.join(map(str, a.frac))} --repeats "
             f"{a.repeats}` on {rec['device']}: device-event times in ms, median (min .. max) of {a.repeats} repeats "
             "after a warm pass (save / load: wall clock).", "",
             f"`ops.index_build` over all {n} rows: {cell(rec['build'])} ms; the index keeps {index.nbytes / 1e9:.3f} GB.",
             "", "| add | whole | top1 | order | fill | repack | pack | repack GB/s | whole / build |",
             "|---|---|---|---|---|---|---|---|---|"]
    nv = int(index.offsets[-1])
    rec["add"], rec["remove"] = [], []
    for f in a.frac:
        n1 = int(round(f * n))
        st = add_phases(index, X[n : n + n1], C, pk, a.repeats)
        gbs = _moved_bytes(index, nv) / (st["repack"]["median_ms"] / 1e3) / 1e9
        one = {"frac": f, "rows": n1, **st, "repack_bytes": _moved_bytes(index, nv), "repack_gb_per_s": round(gbs, 1),
               "add_over_build": round(st["add"]["median_ms"] / rec["build"]["median_ms"], 4)}
        rec["add"].append(one)
        print(json.dumps({"add": one}), flush=True)
        lines.append(f"| {n1} rows ({f:g} N) | {cell(st['add'])} | {cell(st['top1'])} | {cell(st['order'])} | "
                     f"{cell(st['fill'])} | {cell(st['repack'])} | {cell(st['pack'])} | {gbs:.0f} | {one['add_over_build']:.3f} |")
    lines += ["", "| remove | whole | order | fill | repack | repack GB/s | whole / build |", "|---|---|---|---|---|---|---|"]
    for f in a.frac:
        ids = torch.randperm(n, generator=g)[: int(round(f * n))].to(dev)
        st, removed = remove_phases(index, ids, a.repeats)
        moved = _moved_bytes(index, nv - removed)
        gbs = moved / (st["repack"]["median_ms"] / 1e3) / 1e9
        one = {"frac": f, "ids": int(ids.numel()), "removed": removed, **st, "repack_bytes": moved,
               "repack_gb_per_s": round(gbs, 1),
               "remove_over_build": round(st["remove"]["median_ms"] / rec["build"]["median_ms"], 4)}
        rec["remove"].append(one)
        print(json.dumps({"remove": one}), flush=True)
        lines.append(f"| {ids.numel()} ids ({f:g} N) | {cell(st['remove'])} | {cell(st['order'])} | {cell(st['fill'])} | "
                     f"{cell(st['repack'])} | {gbs:.0f} | {one['remove_over_build']:.3f} |")
    # save / load through the public class
    cix = mikmeans.ClusterIndex(km, index, 0, None)
    where = a.dir or tempfile.mkdtemp(prefix="mikmeans-index-")
    ts, tl = [], []
    try:
        for r in range(a.repeats + 1):
            _, s = _wall(lambda: cix.save(where))
            back, l = _wall(lambda: mikmeans.ClusterIndex.load(where, km))
            if r:
                ts.append(s)
                tl.append(l)
            del back
    finally:
        if a.dir is None:
            shutil.rmtree(where, ignore_errors=True)
    rec["save"], rec["load"] = _stat(ts), _stat(tl)
    lines += ["", f"`ClusterIndex.save`: {cell(rec['save'])} ms; `ClusterIndex.load`: {cell(rec['load'])} ms (wall clock, "
                  f"{index.nbytes / 1e9:.3f} GB of tensors)."]
    lines += ["", "```", json.dumps(rec), "```"]
    print(json.dumps(rec), flush=True)
    for path, text in ((a.out, "\n".join(lines) + "\n"), (a.json, json.dumps(rec) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w", encoding="utf-8") as fh:
                fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
