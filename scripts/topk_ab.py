"""The fused top-m kernel (ops.topk, csrc/topk.hip) against the only route there was before it:
ops.transform(squared=True) + torch.topk(m, largest=False) in row blocks of 256 MB of
distances.  One process, one serving pack, the arms interleaved (order reversed every other
round); both arms include the row norms.  One JSON line per shape."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from mikmeans import ops
from mikmeans.data import blobs as B

SHAPES = [(1_000_000, 128, 1024, 8), (1_000_000, 128, 1024, 32), (1_000_000, 64, 4096, 8)]


def route(X, cen, m, pack):
    rows = max(1, (1 << 26) // cen.shape[0])
    idx = torch.empty((X.shape[0], m), dtype=torch.int64, device=X.device)
    d2 = torch.empty((X.shape[0], m), dtype=torch.float32, device=X.device)
    for s in range(0, X.shape[0], rows):
        t = ops.transform(X[s : s + rows], cen, squared=True, pack=pack).topk(m, dim=1, largest=False)
        d2[s : s + rows] = t.values
        idx[s : s + rows] = t.indices
    return idx, d2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for n, d, k, m in SHAPES:
        X = B.make_blobs(n, d, k, seed=1, dtype=torch.bfloat16, device="cuda")
        cen = X[:k].float()
        pack = ops.pack_centers(cen, d, torch.bfloat16, "cuda")
        arms = {"fused": lambda: ops.topk(X, cen, m, pack=pack), "transform_topk": lambda: route(X, cen, m, pack)}
        fi, fd = arms["fused"]()
        ri, rd = arms["transform_topk"]()
        same = bool(torch.equal(fd, rd))           # (torch.topk orders equal distances as it likes)
        t = {name: [] for name in arms}
        for rnd in range(a.rounds):
            for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                arms[name]()
                ev[0].record()
                for _ in range(a.reps):
                    arms[name]()
                ev[1].record()
                torch.cuda.synchronize()
                t[name].append(ev[0].elapsed_time(ev[1]) / a.reps)
        med = {name: statistics.median(v) for name, v in t.items()}
        print(json.dumps({"n": n, "d": d, "k": k, "m": m, "dtype": "bfloat16", "distances_equal": same,
                          "fused_ms": round(med["fused"], 3), "transform_topk_ms": round(med["transform_topk"], 3),
                          "fused_speedup": round(med["transform_topk"] / med["fused"], 3),
                          "all_ms": {name: [round(x, 3) for x in v] for name, v in t.items()}}), flush=True)
        del X, fi, fd, ri, rd


if __name__ == "__main__":
    main()
