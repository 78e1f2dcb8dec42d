#!/usr/bin/env python3
"""One-process A/B of the production kernels against the SAME kernels at a git ref.

No hand-maintained kernel copies: ``build`` checks ``mikmeans/csrc`` out of a git ref
(``git archive``) and compiles it, with the production build (``mikmeans/_build.py``),
into a separately named extension module under ``scripts/abbin/`` (in-tree, so it
travels to the GPU box; built here on the CPU).  ``run`` (GPU) loads the current
``mikmeans._C`` and that module side by side and times their kernels on identical
inputs in interleaved rounds, so box-to-box clock differences cancel.

  python scripts/ab_ext.py build HEAD~1            # prints the module path
  python scripts/ab_ext.py run scripts/abbin/_C_ab_<sha>.so --n 20000000 --d 128 --k 1024
  python scripts/ab_ext.py run scripts/abbin/_C_ab_<sha>.so --what rows   # the row kernels, bit for bit
  python scripts/ab_ext.py run scripts/abbin/_C_ab_<sha>.so --what assign --mode bounded   # an assign mode, bit for bit
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tarfile
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
ABBIN = ROOT / "scripts" / "abbin"


def cmd_build(ref: str) -> Path:
    from mikmeans import _build

    sha = subprocess.run(["git", "-C", str(ROOT), "rev-parse", ref], check=True, capture_output=True,
                         text=True).stdout.strip()[:12]
    src_root = ROOT / "build" / "ab" / sha
    csrc = src_root / "mikmeans" / "csrc"
    if not csrc.exists():
        src_root.mkdir(parents=True, exist_ok=True)
        with tempfile.NamedTemporaryFile(suffix=".tar") as tf:
            subprocess.run(["git", "-C", str(ROOT), "archive", "-o", tf.name, sha, "mikmeans/csrc"], check=True)
            with tarfile.open(tf.name) as t:
                t.extractall(src_root)
    ABBIN.mkdir(parents=True, exist_ok=True)
    module = f"_C_ab_{sha}"
    out = ABBIN / f"{module}.so"
    _build.build(verbose=False, csrc=csrc, build_dir=src_root / "obj", out=out, module=module)
    (ABBIN / f"{module}.json").write_text(json.dumps({"ref": ref, "sha": sha}))
    print(out)
    return out


def load_module(path: str):
    import torch  # noqa: F401  (torch's HIP runtime first)

    name = Path(path).stem
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _timed(fn, reps):
    import torch

    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def _rows_cases(torch, dev):
    """The row kernels' cases (csrc/rows.hip, csrc/kpp.hip, the partition of csrc/ivf.hip, the two
    radix selects): ``(kernel, case, prep)`` with ``prep(m) -> (run, outputs)`` on module ``m``;
    ``run()`` launches the case from the same input state every time, ``outputs`` are what it
    wrote.  Inputs come from a seed of the case's own, so every module sees the same."""
    i32, i64, f32, f64 = torch.int32, torch.int64, torch.float32, torch.float64

    def gen(seed):
        return torch.Generator(device=dev).manual_seed(seed)

    def new(shape, dtype, fill=0):
        return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device=dev)

    ns = (1, 65, 4097, 300_001)
    for dt in (torch.bfloat16, f32):
        v = 8 if dt == torch.bfloat16 else 4
        for D in (4, 20, 128, 1024):
            Dp = -(-D // v) * v
            for n in ns:
                tag = f"{'bf16' if dt == torch.bfloat16 else 'f32'} n={n} D={D}"
                g = gen(n + D)
                X = torch.zeros((n, Dp), dtype=dt, device=dev)
                X[:, :D] = (torch.randn((n, D), generator=g, device=dev) * 3).to(dt)
                X[n // 2] = 0     # (a zero row: the normalise's floor, a zero distance)

                def smp(m, X=X, n=n):
                    out, xn, idx = torch.empty_like(X), new(n, f32), new(n, i64)
                    return (lambda: m.sample_rows(X, out, n, 99, 1, 7, xn, idx)), (out, xn, idx)

                def nrm(m, X=X, n=n):
                    Y, xn = X.clone(), new(n, f32)

                    def run():
                        Y.copy_(X)
                        m.row_normalize(Y, xn)
                    return run, (Y, xn)

                rpb = 1024
                nb = -(-n // rpb)
                c3 = [X[(j * 7919) % n].float().contiguous() for j in range(3)]

                def kd2(m, X=X, n=n, nb=nb, c3=c3):   # the first pass, two pruned passes, one unpruned
                    d2, d2u, own = new(n, f32), new(n, f32), new(n, i32)
                    bs = [new(nb, f64) for _ in range(4)]
                    cc = [new(3, f32), new(3, f32)]   # (one slot a centre, as the seeding holds them)
                    C = torch.stack(c3)

                    def run():
                        own.zero_()
                        m.kpp_d2(X, c3[0], True, d2, bs[0], rpb)
                        d2u.copy_(d2)
                        m.kpp_d2(X, c3[1], False, d2u, bs[3], rpb)
                        m.kpp_cc(C, 1, c3[1], cc[0])
                        m.kpp_d2(X, c3[1], False, d2, bs[1], rpb, own, cc[0], 1, 1)
                        m.kpp_cc(C, 2, c3[2], cc[1])
                        m.kpp_d2(X, c3[2], False, d2, bs[2], rpb, own, cc[1], 2, 2)
                    return run, (d2, d2u, own, *bs, *cc)

                def ksm(m, X=X, n=n, nb=nb):
                    d2 = torch.rand(n, generator=gen(n), device=dev) ** 4
                    d2[::3] = 0
                    pad = torch.zeros(nb * rpb, dtype=f64, device=dev)
                    pad[:n] = d2.double()
                    bsum = pad.view(nb, rpb).sum(1)
                    crow, idx = new(X.shape[1], f32), new(1, i64)
                    tgt = torch.tensor([0.37], dtype=f64, device=dev)
                    return (lambda: m.kpp_sample(bsum, d2, rpb, tgt, X, crow, idx, 1, None, 0)), (crow, idx)

                yield "sample_rows", tag, smp
                yield "row_normalize", tag, nrm
                yield "kpp_d2 + kpp_cc", tag, kd2
                yield "kpp_sample", tag, ksm
                del X
    for n in ns + (4_198_401,):
        g = gen(n)
        if n <= ns[-1]:
            a_, w_ = torch.randn(n, generator=g, device=dev) * 3, torch.randn(n, generator=g, device=dev)

            def wd(m, a_=a_, w_=w_):
                out, scr = new(1, f64), new(m.WDOT_SCRATCH, f64)

                def run():
                    out.fill_(0.37)
                    m.wdot(a_, w_, out, scr)
                return run, (out, scr)

            d2 = torch.rand(n, generator=g, device=dev) ** 4 * 50
            psi = d2.double().sum().reshape(1)

            def kps(m, d2=d2, psi=psi, n=n):
                cand = new(n, torch.uint8)
                return (lambda: m.kpar_select(d2, (1 << 32) - 5, psi, 2000.0, 11, 3, cand)), (cand,)

            yield "wdot", f"n={n}", wd
            yield "kpar_select", f"n={n}", kps
        flags = (torch.rand(n, generator=g, device=dev) < 0.3).to(torch.uint8)

        def cmp_(m, flags=flags, n=n):
            rows, cnt, scr = new(n, i64, -7), new(1, i64, -1), new(max(1, m.compact_blocks(n)), i64)
            return (lambda: m.compact(flags, rows, cnt, scr)), (rows, cnt, scr)

        yield "compact", f"n={n}", cmp_
    for M in (257, 70_000):
        g = gen(M)
        Ct = torch.randn((8, M), generator=g, device=dev)
        w = torch.randint(0, 20, (M,), generator=g, device=dev).double()
        u = torch.rand(3, generator=g, dtype=f64, device=dev)

        def wk(m, Ct=Ct, w=w, u=u, M=M):
            d2, cum, part = new(M, f64), new(M, f64), new(-(-M // 256), f64)
            state, out, init = new(2, i64), new((3, 8), f32), torch.tensor([-1, 0], device=dev)

            def run():
                d2.fill_(float("inf"))
                state.copy_(init)
                m.wkpp(Ct, w, d2, cum, part, u, state, out, 3)
            return run, (cum, part, out, state, d2)

        yield "wkpp", f"M={M}", wk
    for n, K in [(n, 37) for n in ns] + [(70_001, 1024)]:
        lab = torch.randint(-1, K + 1, (n,), generator=gen(n + K), device=dev).to(i32)

        def pt(m, lab=lab, n=n, K=K):
            order, offs, rpos = new(n, i64), new(K + 1, i64), new(n, i64)
            cells = new(K * m.partition_blocks(n, K), i64)
            return (lambda: m.partition(lab, K, order, offs, cells, rpos)), (order, offs, cells, rpos)

        yield "partition", f"n={n} K={K}", pt
    for K in ns[:3]:
        g = gen(K)
        t0 = torch.randint(0, 1000, (K, 256), generator=g, device=dev) * (torch.rand((K, 1), generator=g, device=dev) > 0.2)
        t1 = torch.randint(0, 1000, (K, 3, 256), generator=g, device=dev)
        q = torch.tensor([0.1, 0.5, 0.99], dtype=f64, device=dev)

        def qs(m, t0=t0, t1=t1, K=K):
            pre, rank, cnt = new((K, 3), i32), new((K, 3), i64), new(K, i64)
            p0, r0 = new((K, 3), i32), new((K, 3), i64)

            def run():
                m.quantile_select(t0, q, pre, rank, cnt, 0)
                p0.copy_(pre)
                r0.copy_(rank)
                m.quantile_select(t1, q, pre, rank, cnt, 1)
            return run, (pre, rank, cnt, p0, r0)

        s0 = torch.randint(0, 50, (K, 256), generator=g, device=dev).to(i32)
        s1 = torch.randint(0, 50, (K, 256), generator=g, device=dev).to(i32)

        def isel(m, s0=s0, s1=s1, K=K):
            pre, st = new(K, i32), [new(K, i64) for _ in range(3)]
            first = [new(K, i32)] + [new(K, i64) for _ in range(3)]

            def run():
                m.ivf_select(s0, pre, *st, 100, 0)
                for d, s in zip(first, [pre, *st]):
                    d.copy_(s)
                m.ivf_select(s1, pre, *st, 100, 1)
            return run, (pre, *st, *first)

        yield "quantile_select", f"K={K}", qs
        yield "ivf_select", f"nq={K}", isel


def cmd_rows(mods, a) -> int:
    """``--what rows``: every case on every module, outputs compared bit for bit with the head's
    (floats as integer views) and timed in interleaved rounds; one JSON line, a kernel a key."""
    import torch

    dev = torch.device("cuda")
    ints = {torch.float32: torch.int32, torch.float64: torch.int64, torch.bfloat16: torch.int16}
    res = {}
    for kernel, case, prep in _rows_cases(torch, dev):
        k = res.setdefault(kernel, {"cases": 0, "differ": [], "rounds": {t: [0.0] * a.rounds for t in mods}})
        k["cases"] += 1
        runs, snap = {}, {}
        for tag, m in mods.items():
            runs[tag], outs = prep(m)
            runs[tag]()          # (also the warm-up)
            torch.cuda.synchronize()
            snap[tag] = [o.view(ints.get(o.dtype, o.dtype)).clone() for o in outs]
        for tag in mods:
            if not all(torch.equal(x, y) for x, y in zip(snap[tag], snap["head"])):
                k["differ"].append(f"{tag}: {case}")
        for r in range(a.rounds):
            for tag in mods:
                k["rounds"][tag][r] += statistics.median(_timed(runs[tag], a.reps))
        del runs, snap
    out = {"what": "rows", "rounds": a.rounds, "reps": a.reps, "kernels": {}}
    for kernel, k in res.items():
        # per round, the sum over the kernel's cases of the round's median; their median and spread
        out["kernels"][kernel] = {"cases": k["cases"], "outputs_equal_head": not k["differ"], "differ": k["differ"],
                                  "variants": {tag: {"median_ms": round(statistics.median(v), 4),
                                                     "round_median_spread_ms": round(max(v) - min(v), 4)}
                                               for tag, v in k["rounds"].items()}}
    print(json.dumps(out), flush=True)
    return 0 if all(k["outputs_equal_head"] for k in out["kernels"].values()) else 1


ASSIGN_MODES = ("plain", "noxn", "split", "gathered", "bounded", "persist")


def _assign_cases(mode):
    """``--what assign --mode``: the small cases of a mode, ``(dtype, D, chunks, outlier, variants)``.
    ``chunks``: K in chunks of centres (1, or 17: an odd count, so the persistent ring's slot
    parity flips, and a last key segment of fewer than 16 tiles); ``outlier``: row 3 scaled x64
    (its workgroup takes per-point seed offsets); ``variants``: A/B switches set on each module
    (upper case) and options of the case (``oseed``: pass, or withhold, the full pass's seed offsets).
    Across the modes every built width, a D below its padded width, both offset modes and
    every assign switch occur at least once."""
    bf, f32 = "bf16", "f32"
    if mode == "plain":
        for dt, ds in ((bf, (32, 64, 128, 256, 384, 512, 768, 1024)), (f32, (32, 128, 512, 1024))):
            for D in ds:
                yield dt, D, 1, False, {}
                yield dt, D, 17, True, {}
        yield bf, 104, 17, False, {}           # (D below the padded width: the column-checked loads)
        yield f32, 100, 17, True, {}
        for v in (0, 1):
            yield bf, 64, 17, bool(v), {"ASSIGN_VARG": v}
            yield bf, 128, 17, bool(v), {"ASSIGN_PMAJ": v}
            yield f32, 128, 17, False, {"ASSIGN_PMAJ": v}
        yield bf, 128, 34, False, {"ASSIGN_GEOM": 1}    # (32 KiB chunks: 17 of them)
        yield bf, 128, 17, True, {"ASSIGN_GEOM": 2}
        yield bf, 256, 17, False, {"ASSIGN_GEOM": 1}
    elif mode == "noxn":
        for dt, D, o in ((bf, 128, False), (bf, 64, True), (bf, 512, False), (f32, 128, False), (f32, 100, True)):
            yield dt, D, 17, o, {}
    elif mode == "split":
        for dt, D, o in ((bf, 128, False), (bf, 128, True), (bf, 104, True), (bf, 512, False), (f32, 128, False)):
            yield dt, D, 17, o, {}
        yield bf, 64, 17, False, {"ASSIGN_VARG": 1}
    elif mode == "gathered":
        for dt, D, o in ((bf, 128, False), (bf, 256, True), (bf, 768, False), (f32, 32, False)):
            yield dt, D, 17, o, {}
        yield bf, 64, 17, False, {"ASSIGN_VARG": 1, "oseed": True}    # (the value-only argmin under per-row offsets)
        yield bf, 128, 17, False, {"oseed": True}
    elif mode == "bounded":
        for dt, D, o in ((bf, 32, False), (bf, 128, False), (bf, 128, True), (bf, 256, True), (bf, 384, False),
                         (f32, 128, False)):
            yield dt, D, 17, o, {}
        for v in (0, 1):                       # (1: the full pass ranks by value, so the exact bf16 epilogue)
            yield bf, 64, 17, bool(v), {"ASSIGN_VARG": v}
        yield bf, 128, 17, False, {"ASSIGN_TOP2_GEOM": 0}
        for o in (False, True):                # (no seed offsets: the TOP2 epilogues under the shared / per-point offsets)
            yield bf, 128, 17, o, {"oseed": False}
            yield bf, 64, 17, o, {"ASSIGN_VARG": 1, "oseed": False}
    elif mode == "persist":
        for chunks, o in ((1, False), (17, False), (17, True)):
            yield bf, 128, chunks, o, {"ASSIGN_PERSIST": 5}


def _assign_prep(torch, m, mode, dt, X, Cen, code, dpad, K, opts):
    """One module's inputs and outputs of an assign in ``mode`` on rows X: ``(run, outputs)``; its own
    pack, norms, scratch and outputs, and the same input state before every ``run()``."""
    dev, n = X.device, X.shape[0]
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    kpad = m.assign_kpad(code, dpad, K)
    pack = torch.zeros(kpad * dpad, dtype=dt, device=dev)
    cn = torch.zeros(m.assign_cn_len(kpad), dtype=f32, device=dev)
    m.finalize(0, None, Cen, None, None, None, pack, cn, None, None, dpad, kpad)
    xn = torch.empty(n, dtype=f32, device=dev)
    m.row_sqnorm(X, xn)
    lab, mind = torch.empty(n, dtype=i32, device=dev), torch.empty(n, dtype=f32, device=dev)
    slots = torch.empty(m.NSLOT * m.SLOT_STRIDE, dtype=torch.float64, device=dev)
    ub, lb = torch.empty(n, dtype=f32, device=dev), torch.empty(n, dtype=f32, device=dev)
    args, kw, outs = [X, pack, cn, xn, lab, mind, slots, kpad, dpad, True], {}, [lab, mind, slots]
    if mode == "noxn":
        args[3], args[5], outs = None, None, [lab, slots]
    if mode == "split":
        kw["keys"] = torch.full((n,), -1, dtype=i64, device=dev)
        outs.append(kw["keys"])
    if mode == "gathered":     # a permutation with repeats, and a device count short of its length
        g = torch.Generator(device=dev).manual_seed(n)
        rows = torch.randperm(n, generator=g, device=dev)
        rows[1::5] = rows[0::5][: rows[1::5].numel()]
        kw.update(rows=rows, count=torch.tensor([n - 5], dtype=i64, device=dev))
    if mode == "bounded":      # two rows of three, outputs at their X rows, the full pass's seed offsets
        kw.update(rows=torch.arange(n, device=dev)[torch.arange(n, device=dev) % 3 != 0].contiguous(), ub=ub, lb=lb,
                  scatter=True)
        outs += [ub, lb]
    if dt == torch.bfloat16 and opts.get("oseed", mode == "bounded"):
        kw["oseed"] = torch.empty(n, dtype=f32, device=dev)
        m.seed_offsets(xn, kw["oseed"], m.assign_block_rows(code, dpad, kpad))

    def run(reset=True):
        if reset:
            lab.fill_(7)
            mind.fill_(-1.0)
            slots.zero_()
            ub.zero_()
            lb.zero_()
        m.assign(*args, **kw)
    return run, outs


def cmd_assign_modes(mods, a) -> int:
    """``--what assign --mode M``: every output of every module (labels, mind, ub / lb, the slot
    words, the keys scratch) against the head's, bit for bit -- on the mode's small cases, or,
    with ``--n`` / ``--d`` / ``--k``, on that one shape, timed in interleaved rounds."""
    import torch

    from mikmeans.ops import native

    dev = torch.device("cuda")
    ints = {torch.float32: torch.int32, torch.float64: torch.int64}
    timed = a.n is not None or a.d is not None or a.k is not None
    if timed:
        cases = [(a.dtype, a.d or 128, None, False, {"ASSIGN_PERSIST": 1} if a.mode == "persist" else {})]
    else:
        cases = list(_assign_cases(a.mode))
    differ, res = [], {"what": "assign", "mode": a.mode, "cases": len(cases)}
    for dts, D, chunks, outlier, variants in cases:
        opts = {k: v for k, v in variants.items() if k.islower()}
        variants = {k: v for k, v in variants.items() if not k.islower()}
        dt = torch.bfloat16 if dts == "bf16" else torch.float32
        code, v = native.dtype_code(dt), (8 if dts == "bf16" else 4)
        Dp = -(-D // v) * v
        dpad = native.dpad_for(Dp, dt)
        tag = f"{dts} D={D} chunks={chunks} outlier={int(outlier)} {variants} {opts}"
        runs, snap = {}, {}
        for name, m in mods.items():
            names = m.variant_names()
            for kname, kv in variants.items():
                m.set_variant(names.index(kname), kv)
            # (the chunk and the workgroup's rows under the case's switches, from the module itself)
            K = (a.k or 1024) if timed else chunks * m.assign_kpad(code, dpad, 1)
            kpad = m.assign_kpad(code, dpad, K)
            groups = 11 if a.mode == "persist" else 3
            n = (a.n or 20_000_000) if timed else groups * m.assign_block_rows(code, dpad, kpad) + 17
            g = torch.Generator(device=dev).manual_seed(D + K)
            X = torch.zeros((n, Dp), dtype=dt, device=dev)
            X[:, :D] = (torch.randn((n, D), generator=g, device=dev) * 3).to(dt)
            if outlier:
                X[3] *= 64
            Cen = torch.zeros((K, Dp), dtype=torch.float32, device=dev)
            Cen[:, :D] = torch.randn((K, D), generator=g, device=dev) * 3
            runs[name], outs = _assign_prep(torch, m, a.mode, dt, X, Cen, code, dpad, K, opts)
            runs[name]()
            torch.cuda.synchronize()
            snap[name] = [o.view(ints.get(o.dtype, o.dtype)).clone() for o in outs]
            if not timed:
                for kname in variants:
                    m.set_variant(names.index(kname), -1)
                del X, Cen
        for name in mods:
            if not all(torch.equal(x, y) for x, y in zip(snap[name], snap["head"])):
                differ.append(f"{name}: {tag}")
        # (a guard on the comparison itself: the head's labels are no constant)
        res["min_distinct_labels"] = min(res.get("min_distinct_labels", 1 << 30), int(snap["head"][0].unique().numel()))
        if timed:
            ts = {name: [] for name in mods}
            for _ in range(a.rounds):
                for name in mods:
                    ts[name] += _timed(lambda r=runs[name]: r(False), a.reps)   # (the launch alone)
            res.update(n=n, d=D, k=K, dtype=dts, variants={})
            for name, t in ts.items():
                rmed = [statistics.median(t[i: i + a.reps]) for i in range(0, len(t), a.reps)]
                res["variants"][name] = {"median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                                         "round_median_spread_ms": round(max(rmed) - min(rmed), 4),
                                         "vs_head": round(statistics.median(ts["head"]) / statistics.median(t), 4)}
        del runs, snap
    res.update(outputs_equal_head=not differ, differ=differ)
    print(json.dumps(res), flush=True)
    if res["min_distinct_labels"] <= 1:
        print("every label of a case is the same: the comparison says nothing", file=sys.stderr)
        return 1
    return 0 if not differ else 1


def cmd_run(a) -> int:
    import torch

    from mikmeans.data.blobs import blob_centers, make_blobs
    from mikmeans.models.init import init_random
    from mikmeans.models.lloyd import LloydEngine
    from mikmeans.ops import native
    from mikmeans.parallel import Comm

    mods = {"head": native.require()}
    for p in a.modules:
        meta = Path(p).with_suffix(".json")
        tag = json.loads(meta.read_text())["ref"] if meta.exists() else Path(p).stem
        while tag in mods:   # (the same module twice: an A/A control)
            tag += "'"
        mods[tag] = load_module(p)
    if a.what == "assign" and a.mode is not None:
        return cmd_assign_modes(mods, a)
    a.n, a.d, a.k, a.mode = a.n or 20_000_000, a.d or 128, a.k or 1024, a.mode or "plain"
    if a.what == "rows":   # its own shapes, many and small (--n / --d / --k / --dtype do not apply)
        return cmd_rows(mods, a)
    dt = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    dev = torch.device("cuda")
    comm = Comm.local(dev)
    X = make_blobs(a.n, a.d, a.k, seed=0, dtype=dt, device=dev, centers=blob_centers(a.k, a.d, 10.0, 0, device=dev))
    eng = LloydEngine(X, a.k, comm=comm).set_centers(init_random(X, a.d, a.k, a.n, 0, comm, 0))
    for _ in range(3):
        eng.step()
    Cen = eng.C.contiguous()
    code = native.dtype_code(dt)
    dpad = native.dpad_for(eng.Dp, dt)
    per = {}
    for tag, m in mods.items():
        for kv in filter(None, (a.set or "").split(",")):   # the same A/B switches on every module
            name, v = kv.split("=")
            m.set_variant([x.lower() for x in m.variant_names()].index(name.strip().lower()), int(v))
        kpad = m.assign_kpad(code, dpad, a.k)
        pack = torch.zeros(kpad * dpad, dtype=dt, device=dev)
        cn = torch.zeros(m.assign_cn_len(kpad), dtype=torch.float32, device=dev)
        m.finalize(0, None, Cen, None, None, None, pack, cn, None, None, dpad, kpad)
        lab = torch.empty(a.n, dtype=torch.int32, device=dev)
        mind = torch.empty(a.n, dtype=torch.float32, device=dev)
        slots = torch.zeros(m.NSLOT * m.SLOT_STRIDE, dtype=torch.float64, device=dev)
        per[tag] = dict(m=m, pack=pack, cn=cn, kpad=kpad, lab=lab, mind=mind, slots=slots, ts=[])
        # a module with the per-group seed statistics (group_norm_stats) runs as two arms: with its table
        # (built once, as a fit does) and, "<tag> no table", reducing the norms in every workgroup
        if a.what == "assign" and hasattr(m, "group_norm_stats") and dt == torch.bfloat16 \
                and m.assign_block_rows(code, dpad, kpad) == m.GSTATS_ROWS:
            gs = torch.empty((-(-a.n // m.GSTATS_ROWS), 2), dtype=torch.float32, device=dev)
            m.group_norm_stats(eng.xn, gs, 0)
            per[tag + " no table"] = dict(per[tag], lab=torch.empty_like(lab), mind=torch.empty_like(mind),
                                          slots=torch.zeros_like(slots), ts=[])
            per[tag]["kw"] = {"gstats": gs}

    def run_assign(t):
        t["m"].assign(eng.X, t["pack"], t["cn"], eng.xn, t["lab"], t["mind"], t["slots"], t["kpad"], dpad, True,
                      None, **t.get("kw", {}))

    if a.what == "update":   # one set of inputs per --mode (the head's), the same for every module
        from mikmeans import ops

        g = torch.Generator(device=dev).manual_seed(1)
        uw = torch.rand(a.n, generator=g, device=dev) + 0.5 if a.mode == "weighted" else None
        ucol, ucnt = ops.fixed_exps(eng.X, uw) if uw is not None else (eng.col_exp, eng.cnt_exp)
        ukw = {}
        if a.mode == "resid":      # the lo pass of two columns
            ukw["col_exp2"] = torch.full_like(ucol, -1000)
            ukw["col_exp2"][[0, eng.Dp // 2]] = ucol[[0, eng.Dp // 2]] + 20
        if a.mode == "gather":     # a permutation with repeats
            ukw["rows"] = torch.randperm(a.n, generator=g, device=dev)
            ukw["rows"][1::5] = ukw["rows"][0::5][: ukw["rows"][1::5].numel()]
        if a.mode == "delta":      # every tenth row came from the next label
            prev = eng.labels.clone()
            prev[::10] = (prev[::10] + 1) % a.k
            ulist = torch.empty((a.n // 10 + 8, 2), dtype=torch.int32, device=dev)
            ucount = torch.zeros(1, dtype=torch.int32, device=dev)
            mods["head"].label_delta(eng.labels, prev, ulist, ucount)

    def run_update(t):   # one M-step pass on the engine's labels into each module's own slab
        m = t["m"]
        if "slab" not in t:
            t["nch"] = m.update_n_chunks(code, a.k, eng.Dp, a.n, a.mode in ("weighted", "delta"))
            # (zeros: the residual pass leaves the slices without a wide column unwritten)
            t["slab"] = torch.zeros(t["nch"] * a.k * eng.Dp, dtype=torch.int64, device=dev)
            t["cnt"] = torch.zeros(t["nch"] * a.k, dtype=torch.int64, device=dev)
            t["cc"] = torch.zeros(1, dtype=torch.int32, device=dev)
        if a.mode == "delta":
            m.update_delta(eng.X, eng.labels, a.k, t["slab"], t["cnt"], t["nch"], None, ucol, ucnt, ulist, ucount)
        else:
            m.update(eng.X, eng.labels, a.k, t["slab"], t["cnt"], t["nch"], uw, ucol, ucnt, a.mode == "clamp",
                     clamp_count=t["cc"] if a.mode == "clamp" else None, **ukw)

    def run_blobs(t):    # the on-device generator (+ fused row norms) into each module's own buffer
        if "bx" not in t:
            t["bx"] = torch.empty_like(eng.X)
            t["bn"] = torch.empty(a.n, dtype=torch.float32, device=dev)
            t["bc"] = blob_centers(a.k, a.d, 10.0, 0, device=dev)
        t["m"].blobs(t["bx"], 0, t["bc"], 1.0, 7, None, t["bn"])

    def run_colstats(t):  # the setup pass: column statistics + fused row norms
        m = t["m"]
        t.setdefault("cs", (torch.zeros(eng.Dp, dtype=torch.int32, device=dev),
                            torch.zeros(3 * eng.Dp, dtype=torch.float64, device=dev),
                            torch.zeros(eng.Dp, dtype=torch.int64, device=dev),
                            torch.zeros(eng.Dp, dtype=torch.int32, device=dev),
                            torch.empty(a.n, dtype=torch.float32, device=dev)))
        out, fst, nnz, lowbit, xn = t["cs"]
        out.zero_(); nnz.zero_(); lowbit.fill_(1 << 30)
        m.col_absmax(eng.X, out, fst, nnz, lowbit, xn)

    def run_rownorms(t):  # the plain row-norm pass
        t.setdefault("rn", torch.empty(a.n, dtype=torch.float32, device=dev))
        t["m"].row_sqnorm(eng.X, t["rn"])

    def run_transform(t):  # squared distances to every centre, [n, k]
        t.setdefault("out", (torch.empty((a.n, a.k), dtype=torch.float32, device=dev),))
        t["m"].transform(eng.X, t["pack"], t["cn"], a.k, t["kpad"], dpad, eng.xn, t["out"][0], True)

    def run_topk(t):       # the --m nearest centres of every row
        t.setdefault("out", (torch.empty((a.n, a.m), dtype=torch.float32, device=dev),
                             torch.empty((a.n, a.m), dtype=torch.int32, device=dev)))
        t["m"].topk(eng.X, t["pack"], t["cn"], a.k, t["kpad"], dpad, eng.xn, *t["out"])

    if a.what in ("ivf_scan", "ivf_range"):   # one index, one set of probes and pairs (the head's) for every module
        from mikmeans import ops
        from mikmeans.ops import index as ix

        head = mods["head"]
        index, Q = ix.index_build(eng.X, Cen), eng.X[: a.nq]
        probes, npairs = ops.topk(Q, Cen, a.nprobe)[0], Q.shape[0] * a.nprobe

        def walk(P, *mid):   # the leading arguments of ivf_scan / ivf_range
            porder, poff, icum, max_items = ix.pair_items(index, probes, P)
            return (Q, ops.row_sqnorm(Q), *mid, index.pack, index.cn, index.offsets, index.tile_offsets, index.order,
                    porder, poff, icum, a.nprobe, dpad, P, max_items)

        scan = walk(head.ivf_scan_blocks(code, dpad, a.m, npairs))
    if a.what == "ivf_range":   # the radius: the head scan's m-th key per query; base: the head's counts
        keys = torch.empty((npairs, a.m), dtype=torch.int64, device=dev)
        head.ivf_scan(*scan, keys)
        kth = keys.view(Q.shape[0], a.nprobe * a.m).sort(dim=1).values[:, a.m - 1]
        r2 = torch.nan_to_num(ix.index_decode(kth)[1], nan=0.0).contiguous()   # (fewer than m rows probed: 0)
        rng = walk(head.ivf_range_blocks(code, dpad, npairs), r2)
        counts = torch.zeros(npairs, dtype=torch.int64, device=dev)
        head.ivf_range(*rng, counts)
        end = torch.cumsum(counts, 0)
        rbase, total = end - counts, int(end[-1])

    def run_ivf_scan(t):   # the --m nearest indexed rows of every (query, probed list) pair
        t.setdefault("out", (torch.empty((npairs, a.m), dtype=torch.int64, device=dev),))
        t["m"].ivf_scan(*scan, t["out"][0])

    def run_ivf_range(t):  # the count pass, then the fill pass: every row within the radius, per pair
        t.setdefault("out", (torch.zeros(npairs, dtype=torch.int64, device=dev),
                             torch.zeros(total, dtype=torch.int64, device=dev)))
        t["m"].ivf_range(*rng, t["out"][0])
        if total:
            t["m"].ivf_range(*rng, t["out"][0], rbase, t["out"][1])

    fn = {"update": run_update, "blobs": run_blobs, "colstats": run_colstats, "rownorms": run_rownorms,
          "transform": run_transform, "topk": run_topk, "ivf_scan": run_ivf_scan,
          "ivf_range": run_ivf_range}.get(a.what, run_assign)
    for t in per.values():          # warm-up (kernel attributes, code objects)
        fn(t)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for t in per.values():
            t["ts"] += _timed(lambda t=t: fn(t), a.reps)
    base = per["head"]
    if a.what == "blobs":           # the same rows and norms from every module
        for tag, t in per.items():
            t["same"] = bool(torch.equal(t["bx"], per["head"]["bx"]) and torch.equal(t["bn"], per["head"]["bn"]))
    if a.what == "colstats":        # the same max / counts / norms; the f64 sums to ~1e-12
        h = per["head"]["cs"]
        for tag, t in per.items():
            c = t["cs"]
            t["same"] = bool(torch.equal(c[0], h[0]) and torch.equal(c[2], h[2]) and torch.equal(c[3], h[3])
                             and torch.equal(c[4], h[4]) and torch.allclose(c[1], h[1], rtol=1e-12, atol=0))
            t["fsums_bitwise"] = bool(torch.equal(c[1], h[1]))
    if a.what == "rownorms":        # the same bits from every module
        for tag, t in per.items():
            t["same"] = bool(torch.equal(t["rn"], per["head"]["rn"]))
    if a.what in ("transform", "topk", "ivf_scan", "ivf_range"):   # the same bits from every module
        for tag, t in per.items():
            t["same"] = all(torch.equal(x.view(torch.int32), y.view(torch.int32))
                            for x, y in zip(t["out"], per["head"]["out"]))
    if a.what == "update":          # the same integer sums from every module
        red = {tag: (t["slab"].view(t["nch"], -1).sum(0), t["cnt"].view(t["nch"], -1).sum(0)) for tag, t in per.items()}
        for tag, t in per.items():
            t["same"] = bool(torch.equal(red[tag][0], red["head"][0]) and torch.equal(red[tag][1], red["head"][1]))
    out = {"n": a.n, "d": a.d, "k": a.k, "dtype": a.dtype, "what": a.what,
           **({"mode": a.mode} if a.what == "update" else {}), "variants": {}}
    for tag, t in per.items():
        med = statistics.median(t["ts"])
        # a round's own median, and their spread: the box's round-to-round noise
        rmed = [statistics.median(t["ts"][i : i + a.reps]) for i in range(0, len(t["ts"]), a.reps)]
        out["variants"][tag] = {
            "median_ms": round(med, 4), "min_ms": round(min(t["ts"]), 4),
            "round_median_spread_ms": round(max(rmed) - min(rmed), 4),
            "tflops": round(2.0 * a.n * a.k * a.d / (med * 1e-3) / 1e12, 1),
            "x_TBps": round(a.n * a.d * (2 if a.dtype == "bf16" else 4) / (med * 1e-3) / 1e12, 2),
            "label_mismatch_vs_head": int((t["lab"] != base["lab"]).sum()) if a.what == "assign" else None,
            "outputs_equal_head": t.get("same"),
            **({"fsums_bitwise": t["fsums_bitwise"]} if "fsums_bitwise" in t else {}),
            "vs_head": round(statistics.median(base["ts"]) / med, 4),
        }
    print(json.dumps(out), flush=True)
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build")
    b.add_argument("ref")
    r = sub.add_parser("run")
    r.add_argument("modules", nargs="+")
    r.add_argument("--n", type=int, default=None, help="rows (default 20000000)")
    r.add_argument("--d", type=int, default=None, help="features (default 128)")
    r.add_argument("--k", type=int, default=None, help="centres (default 1024)")
    r.add_argument("--dtype", default="bf16")
    r.add_argument("--set", default=None, help="kernel switches set on every module, e.g. assign_persist=1")
    r.add_argument("--rounds", type=int, default=5)
    r.add_argument("--reps", type=int, default=5)
    r.add_argument("--what", default="assign", choices=["assign", "update", "blobs", "colstats", "rownorms",
                                                        "transform", "topk", "ivf_scan", "ivf_range", "rows"])
    r.add_argument("--mode", default=None,
                   choices=["plain", "weighted", "clamp", "resid", "gather", "delta", *ASSIGN_MODES[1:]],
                   help="update: the pass (each reaches another build of the M-step kernels; default plain).  "
                        "assign: every output against the head's bit for bit, on the mode's small cases "
                        f"({', '.join(ASSIGN_MODES)}) or, with --n / --d / --k, timed on that shape; "
                        "without --mode the plain full pass is timed")
    r.add_argument("--m", type=int, default=8,
                   help="topk / ivf_scan: list length; ivf_range: the radius is the m-th nearest row's distance")
    r.add_argument("--nq", type=int, default=10_000, help="ivf_scan / ivf_range: queries (the first rows)")
    r.add_argument("--nprobe", type=int, default=16, help="ivf_scan / ivf_range: lists probed per query")
    a = ap.parse_args(argv)
    if a.cmd == "run" and a.mode is not None:
        modes = {"assign": ASSIGN_MODES, "update": ("plain", "weighted", "clamp", "resid", "gather", "delta")}
        if a.mode not in modes.get(a.what, ()):
            ap.error(f"--what {a.what} takes no --mode {a.mode}")
    if a.cmd == "build":
        cmd_build(a.ref)
        return 0
    return cmd_run(a)


if __name__ == "__main__":
    sys.exit(main())
