"""A/B of the cluster_report reduce stage: the native quality kernel against the PyTorch
reductions the same numbers took before it (profiles/quality_ab.log).

One process, the arms interleaved inside every repeat, device-event times.  bf16 blobs,
D = 128, K = 1024 true centres, n = 1e6 and 1e7, rows in blocks of 2^22 as
``ops.cluster_quality`` takes them.  Per repeat and arm the top-2 pass is timed apart from the
reduce stage:

* ``native``  -- ``ops.quality_accumulate`` by the launcher's rule (the LDS-private kernel here)
* ``global``  -- the same kernel forced to its global-atomic form (``path=0``)
* ``torch``   -- ``bincount``, three float64 ``index_add_`` (sum a^2, sum a, sum s) and
                 ``scatter_reduce(amax)`` on the top-2 output, with the elementwise float64
                 sqrt / divide they need

Usage: ``python scripts/quality_ab.py [--out profiles/quality_ab.log] [--repeats 7] [--n 1000000 10000000]``
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

D, K = 128, 1024
BLOCK = ops.QUALITY_BLOCK_ROWS


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return out, (e0, e1)


def _ms(pairs):
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs)


def arm_native(X, C, pk, path):
    table = torch.zeros((K, ops.QUALITY_WORDS), dtype=torch.int64, device=X.device)
    tk, rd = [], []
    for s in range(0, X.shape[0], BLOCK):
        (idx, d2), ev = _timed(lambda: ops.topk(X[s : s + BLOCK], C, 2, pack=pk))
        tk.append(ev)
        _, ev = _timed(lambda: ops.quality_accumulate(table, idx, d2, path=path))
        rd.append(ev)
    return table, _ms(tk), _ms(rd)


def arm_torch(X, C, pk):
    dev = X.device
    counts = torch.zeros(K, dtype=torch.int64, device=dev)
    sa2, sa, ss = (torch.zeros(K, dtype=torch.float64, device=dev) for _ in range(3))
    mx = torch.zeros(K, dtype=torch.float32, device=dev)
    tk, rd = [], []

    def reduce(idx, d2):
        k = idx[:, 0].long()
        a2 = d2[:, 0].double()
        counts.add_(torch.bincount(k, minlength=K))
        sa2.index_add_(0, k, a2)
        sa.index_add_(0, k, a2.sqrt())
        ss.index_add_(0, k, 1.0 - (a2 / d2[:, 1].double()).sqrt())
        mx.scatter_reduce_(0, k, d2[:, 0], "amax")

    for s in range(0, X.shape[0], BLOCK):
        (idx, d2), ev = _timed(lambda: ops.topk(X[s : s + BLOCK], C, 2, pack=pk))
        tk.append(ev)
        _, ev = _timed(lambda: reduce(idx, d2))
        rd.append(ev)
    return (counts, sa2, sa, ss, mx), _ms(tk), _ms(rd)


def _stat(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default="profiles/quality_ab.log")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--n", type=int, nargs="+", default=[1_000_000, 10_000_000])
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("quality_ab.py measures on the GPU; none found")
    dev = torch.device("cuda")
    lines = [f"# quality_ab: bf16 blobs D={D} K={K}, row blocks of {BLOCK}, {a.repeats} interleaved repeats, "
             f"{torch.cuda.get_device_name(0)}"]
    for n in a.n:
        X = B.make_blobs(n, D, K, seed=7, dtype=torch.bfloat16, device=dev)
        C = B.blob_centers(K, D, 10.0, 7, device=dev)
        pk = ops.pack_centers(C, D, X.dtype, dev)
        for _ in range(2):                                  # warm every shape and code object
            arm_native(X, C, pk, -1), arm_native(X, C, pk, 0), arm_torch(X, C, pk)
        t = {k: [] for k in ("topk", "native", "global", "torch")}
        for _ in range(a.repeats):
            Tn, tk1, r = arm_native(X, C, pk, -1)
            t["native"].append(r)
            (counts, sa2, sa, ss, mx), tk2, r = arm_torch(X, C, pk)
            t["torch"].append(r)
            Tg, tk3, r = arm_native(X, C, pk, 0)
            t["global"].append(r)
            t["topk"] += [tk1, tk2, tk3]
        # the arms computed the same thing
        rep = ops.quality_decode(Tn, C, X.dtype)
        assert torch.equal(Tn, Tg)
        assert torch.equal(rep["counts"], counts.cpu())
        assert torch.allclose(rep["cluster_inertia"], sa2.cpu(), rtol=1e-10)
        assert torch.allclose(torch.nan_to_num(rep["mean_distance"] * rep["counts"]), sa.cpu(), rtol=1e-10)
        assert torch.equal(Tn[:, 17].cpu().to(torch.int32).view(torch.float32), mx.cpu())   # the largest a^2
        st = {k: _stat(v) for k, v in t.items()}
        rec = {"n": n, "D": D, "K": K, "dtype": "bfloat16", "lds_path": bool(ops.require().quality_uses_lds(
            min(n, BLOCK), K)), **st,
            "reduce_share_of_report": round(st["native"]["median_ms"] / (st["native"]["median_ms"]
                                                                         + st["topk"]["median_ms"]), 4),
            "torch_over_native": round(st["torch"]["median_ms"] / st["native"]["median_ms"], 2)}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del X
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
