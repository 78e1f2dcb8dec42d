"""Command line: ``python -m mikmeans <command>`` (or ``torchrun ... -m mikmeans fit`` for DP).

Commands (the reference's top-bar controls, app.mjs:240-288, as a CLI):

* ``fit``      -- k-means on a file (.npy/.safetensors/.csv) or synthetic blobs; writes a
                  checkpoint (safetensors + JSON), the flat-float ``centroids.json`` and labels
* ``predict``  -- labels of a dataset under a saved model
* ``report``   -- per-cluster quality of a dataset under a saved model (sizes, inertia, radius,
                  simplified silhouette, Davies-Bouldin), as JSON; ``--exemplars M`` adds every
                  cluster's M nearest (``--farthest``: farthest) rows
* ``search``   -- the M rows of a dataset nearest each query, through a saved model's clusters
                  (``--nprobe P`` clusters searched per query; rows and distances as .npz; M up to
                  32, with ``--deep`` up to 2048), or with
                  ``--radius R`` in place of ``--top M`` every row within R of each query (lims, rows
                  and distances as .npz)
* ``blobs``    -- write a synthetic Gaussian-blob dataset
* ``room``     -- the trait-card game headless: seed/populate/auto-assign/dashboard/export/import
* ``session``  -- one participant of a live, replicated room session: found it (hosting the
                  rendezvous store) or join it, submit edits, leave -- the reference's tab
                  joining a room link (app.mjs:70-118)
* ``export``   -- checkpoint -> flat-float centroid JSON or room-export JSON (app.mjs:263-267)
* ``import``   -- room-export JSON -> numeric checkpoint of trait vectors (app.mjs:268-282)
* ``bench``    -- the headline benchmark (same as ``python bench.py``)
* ``launch``   -- run a command as an N-rank job with fresh-process restarts from the last
                  checkpoint (the reference's peers re-meshing after a drop, app.mjs:105-117)
* ``info``     -- device, native extension and build information
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np
import torch


def _comm(device, timeout_s: float = 600.0):
    from .parallel import Comm, set_comm

    c = Comm.from_env(device, timeout_s=timeout_s)
    set_comm(c)
    return c


def _resume_dir(cfg):
    """``--resume auto``: the checkpoint dir when it already holds a checkpoint (a restart)."""
    from .utils.checkpoint import has_checkpoint

    if cfg.resume == "auto":
        return cfg.checkpoint_dir if cfg.checkpoint_dir and has_checkpoint(cfg.checkpoint_dir) else None
    return cfg.resume


def cmd_fit(a) -> int:
    from . import KMeans, MiniBatchKMeans
    from .config import KMeansConfig, resolve_dtype
    from .utils.io import load_points

    cfg = KMeansConfig.from_args(a)
    device = cfg.device or ("cuda" if torch.cuda.is_available() else "cpu")
    comm = _comm(device, cfg.timeout_s)
    resume = _resume_dir(cfg)
    dtype = resolve_dtype(cfg.dtype)
    if a.input:
        X, n, start = load_points(a.input, comm.rank, comm.world)
    else:
        from .data.blobs import make_blobs
        from .parallel import shard_range

        n, d, c = (int(v) for v in a.blobs.split(","))
        start, end = shard_range(n, comm.rank, comm.world)
        X = make_blobs(end - start, d, c, seed=cfg.seed, i0=start, device=comm.device, dtype=dtype)
    if cfg.batch_size > 0:
        km = MiniBatchKMeans(cfg.n_clusters, batch_size=cfg.batch_size, max_iter=cfg.max_iter, init=cfg.init,
                             dtype=dtype, device=comm.device, seed=cfg.seed, comm=comm,
                             init_sampling=cfg.init_sampling)
        if resume and comm.rank == 0:
            print(f"[mikmeans] resuming from {resume}", file=sys.stderr, flush=True)
        # batch rows are drawn by (seed, rank, step): a restart on the same world size
        # continues the interrupted fit exactly
        km.fit(X, resume_from=resume, checkpoint_every=cfg.checkpoint_every, checkpoint_dir=cfg.checkpoint_dir)
    else:
        km = KMeans.from_config(cfg, comm=comm)
        km.device = comm.device
        if resume and comm.rank == 0:
            print(f"[mikmeans] resuming from {resume}", file=sys.stderr, flush=True)
        km.fit(X, resume_from=resume)
    out = Path(a.output) if a.output else None
    if comm.rank == 0:
        rec = {"n_samples": n, "n_clusters": cfg.n_clusters, "world": comm.world}
        if hasattr(km, "inertia_"):
            rec.update(inertia=km.inertia_, n_iter=km.n_iter_, fit_time_s=round(km.fit_time_s_, 4),
                       metrics=km.metrics())
        mp = getattr(km, "memory_plan_", None)
        if mp:
            rec["memory_plan"] = {k: mp[k] for k in ("mode", "peak", "budget", "chunk_rows", "batch_rows")}
        print(json.dumps(rec, default=str))
    if out is not None:
        km.save(out)   # safetensors + state.json + flat centroids.json (mini-batch: + running counts)
        if a.save_labels and hasattr(km, "labels_"):
            lab = km.labels_
            lab = lab.cpu().numpy() if torch.is_tensor(lab) else lab
            np.save(out / f"labels.rank{comm.rank}.npy", lab.astype(np.int32), allow_pickle=False)
    comm.close()
    return 0


def cmd_predict(a) -> int:
    from . import KMeans
    from .utils.io import load_points

    comm = _comm(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    km = KMeans.load(a.model, device=comm.device)
    X, n, start = load_points(a.input, comm.rank, comm.world)
    def _save(path, arr):
        np.save(Path(path).with_suffix(f".rank{comm.rank}.npy") if comm.world > 1 else path, arr,
                allow_pickle=False)

    if a.distances_output and not a.top:
        raise SystemExit("predict: --distances-output needs --top M")
    if a.top:
        # the M nearest centres of every row, nearest first: [n, M] labels (and distances)
        if not 1 <= a.top <= km.cluster_centers_.shape[0]:
            raise SystemExit(f"predict: --top must be in [1, {km.cluster_centers_.shape[0]}], got {a.top}")
        lab, dist = km.predict_topk(X.to(comm.device), a.top)
        dist = dist.cpu().numpy().astype(np.float32)
        if a.distances_output:
            _save(a.distances_output, dist)
    else:
        lab = km.predict(X.to(comm.device))
    lab = lab.cpu().numpy().astype(np.int32)
    if a.output:
        _save(a.output, lab)
    if comm.rank == 0:
        nearest = lab[:, 0] if a.top else lab
        print(json.dumps({"n_samples": n, "counts": np.bincount(nearest, minlength=km.n_clusters).tolist()}))
    comm.close()
    return 0


def cmd_report(a) -> int:
    """Per-cluster quality of a dataset under a saved model (``KMeans.cluster_report``): every
    rank folds its shard, the integer table is all-reduced, rank 0 writes the report.  With
    ``--exemplars M`` the written report also carries every cluster's M nearest (``--farthest``:
    farthest) rows and their distances (``KMeans.cluster_exemplars``, global row indices), with
    ``--quantiles 0.5,0.9,0.99`` every cluster's exact distance quantiles and the rows counted
    (``KMeans.cluster_quantiles``)."""
    from . import KMeans, ops
    from .utils.io import load_points

    if a.exemplars and not 1 <= a.exemplars <= ops.EXEMPLAR_MAX:
        raise SystemExit(f"report: --exemplars must be in [1, {ops.EXEMPLAR_MAX}], got {a.exemplars}")
    qs = None
    if a.quantiles is not None:
        try:
            qs = ops.quantile_levels([float(v) for v in a.quantiles.split(",")])
        except ValueError as e:
            raise SystemExit(f"report: --quantiles takes 1 to {ops.QUANTILE_MAX_Q} comma-separated numbers in "
                             f"[0, 1], got {a.quantiles!r} ({e})")
    comm = _comm(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    km = KMeans.load(a.model, device=comm.device)
    X, n, start = load_points(a.input, comm.rank, comm.world)
    rep = km.cluster_report(X.to(comm.device)).to_dict()
    if a.exemplars:
        from .api import _jsonable

        rows, dist = km.cluster_exemplars(X.to(comm.device), a.exemplars, farthest=a.farthest)
        rep["exemplars"] = _jsonable({"m": int(a.exemplars), "farthest": bool(a.farthest), "rows": rows.cpu(),
                                      "distances": dist.cpu()})
    if qs is not None:
        from .api import _jsonable

        dist, counts = km.cluster_quantiles(X.to(comm.device), qs)
        rep["quantiles"] = _jsonable({"q": qs, "distances": dist.cpu(), "counts": counts.cpu()})
    if comm.rank == 0:
        if a.output:
            Path(a.output).write_text(json.dumps(rep, indent=1))
        print(json.dumps({k: rep[k] for k in ("n_samples", "inertia", "silhouette", "davies_bouldin", "balance")}))
    comm.close()
    return 0


def cmd_search(a) -> int:
    """Nearest-row search through a saved model's clusters (``KMeans.build_index`` /
    ``ClusterIndex.search``, with ``--deep`` ``ClusterIndex.search_deep``): every rank indexes its
    shard of ``--input`` (or, in a one-rank job, loads the saved index of ``--index``), all ranks search the same ``--queries``, the per-rank lists are
    merged and rank 0 writes ``rows`` ([nq, M] int64, global row indices, -1 padded) and ``distances``
    ([nq, M] float32, NaN padded) to ``--output`` (.npz)."""
    from . import KMeans, ops

    if (a.input is None) == (a.index is None):
        raise SystemExit("search: give one of --input X and --index DIR")
    comm = _comm(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    km = KMeans.load(a.model, device=comm.device)
    K = int(km.cluster_centers_.shape[0])
    if (a.top is None) == (a.radius is None):
        raise SystemExit("search: give one of --top M and --radius R")
    if a.radius is not None:
        if a.deep:
            raise SystemExit("search: --deep goes with --top M")
        if a.refine is not None or a.shortlist is not None:
            raise SystemExit("search: --refine and --shortlist go with --top M on a PQ index")
        return _search_radius(a, km, comm)
    most = ops.INDEX_DEEP_MAX_M if a.deep else ops.INDEX_MAX_M
    if not 1 <= a.top <= most:
        raise SystemExit(f"search: --top must be in [1, {most}], got {a.top}")
    if not 1 <= a.nprobe <= K:
        raise SystemExit(f"search: --nprobe must be in [1, {K}], got {a.nprobe}")
    index, n = _search_index(a, km, comm)
    Q = np.load(a.queries, allow_pickle=False)
    refined = {}
    if a.refine is not None or a.shortlist is not None:
        from . import PQIndex

        if not isinstance(index, PQIndex) or a.refine is None:
            raise SystemExit("search: --refine ROWS.npy [--shortlist S] re-ranks a PQ index (--index DIR of index --pq)")
        # (memory-mapped: the rows stay on the host and only the shortlisted ones are read)
        refined = {"refine": np.load(a.refine, mmap_mode="r", allow_pickle=False), "shortlist": a.shortlist}
    try:
        rows, dist = (index.search_deep if a.deep else index.search)(Q, a.top, nprobe=a.nprobe, squared=a.squared,
                                                                     **refined)
    except ValueError as e:
        if not refined:
            raise
        raise SystemExit(f"search: {e}")
    if comm.rank == 0:
        if a.output:
            np.savez(a.output, rows=rows.astype(np.int64), distances=dist.astype(np.float32))
        print(json.dumps({"n_samples": n, "n_queries": int(rows.shape[0]), "top": int(a.top), "nprobe": int(a.nprobe),
                          "found": int((rows >= 0).sum())}))
    comm.close()
    return 0


def _search_index(a, km, comm):
    """``(index, rows)`` of a search: the index built over this rank's shard of ``--input``, or the
    saved one of ``--index`` (``rows``: the dataset's rows, or the row ids the saved index handed out)."""
    from .utils.io import load_points

    if a.index is not None:
        from . import PQIndex

        if PQIndex.saved_at(a.index):          # whichever of the two formats the directory holds
            if a.deep or a.radius is not None:
                raise SystemExit(f"search: {a.index} holds a PQ index, which takes --top M without --deep")
            index = km.load_pq_index(a.index)
        else:
            index = km.load_index(a.index)
        return index, index.n_rows
    X, n, start = load_points(a.input, comm.rank, comm.world)
    return km.build_index(X.to(comm.device)), n


def cmd_index(a) -> int:
    """Build, update and keep a saved model's index (``KMeans.build_index``, ``ClusterIndex.add`` /
    ``remove`` / ``save``): built from ``--input``, or loaded from ``--output`` when that directory
    already holds one; then the row ids of ``--remove`` (.npy, integers) leave, the rows of ``--add``
    join, and the index is written to ``--output``.  Prints ``n_rows``, ``n_indexed``, ``added_first_id``,
    ``removed`` and ``nbytes``."""
    from . import ClusterIndex, KMeans

    from .utils.io import load_points

    comm = _comm(a.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    km = KMeans.load(a.model, device=comm.device)
    if a.pq is not None:
        return _index_pq(a, km, comm)
    if a.input is not None:
        X, n, start = load_points(a.input, comm.rank, comm.world)
        index = km.build_index(X.to(comm.device))
    elif ClusterIndex.saved_at(a.output):
        index = km.load_index(a.output)
    else:
        raise SystemExit(f"index: give --input X to build from: {a.output} holds no index")
    removed = first = None
    if a.remove is not None:
        removed = index.remove(np.load(a.remove, allow_pickle=False))
    if a.add is not None:
        X2, _, _ = load_points(a.add, 0, 1)
        first = index.add(X2)
    index.save(a.output)
    print(json.dumps({"n_rows": index.n_rows, "n_indexed": index.n_indexed, "added_first_id": first,
                      "removed": removed, "nbytes": index.nbytes}))
    comm.close()
    return 0


def _index_pq(a, km, comm) -> int:
    """``index --pq M`` (``KMeans.build_pq_index`` / ``PQIndex.save``): the rows of ``--input`` as M one-byte
    codes a row, written to ``--output``.  Prints ``n_rows``, ``n_indexed``, ``n_subvectors`` and ``nbytes``."""
    from .utils.io import load_points

    if a.input is None or a.add is not None or a.remove is not None:
        raise SystemExit("index: --pq builds from --input X; a PQ index takes no --add or --remove")
    X, n, start = load_points(a.input, comm.rank, comm.world)
    try:
        index = km.build_pq_index(X.to(comm.device), a.pq, train_rows=a.train_rows)
    except ValueError as e:
        raise SystemExit(f"index: {e}")
    index.save(a.output)
    print(json.dumps({"n_rows": index.n_rows, "n_indexed": index.n_indexed, "n_subvectors": index.n_subvectors,
                      "nbytes": index.nbytes}))
    comm.close()
    return 0


def _search_radius(a, km, comm) -> int:
    """``search --radius R`` (``ClusterIndex.range_search``): every row within R of each query among
    its ``--nprobe`` clusters; rank 0 writes ``lims`` ([nq + 1] int64), ``rows`` (int64, global row
    indices) and ``distances`` (float32), query q's hits at ``[lims[q], lims[q + 1])``, nearest first."""
    import math

    K = int(km.cluster_centers_.shape[0])
    if not (math.isfinite(a.radius) and a.radius >= 0):
        raise SystemExit(f"search: --radius must be finite and non-negative, got {a.radius}")
    if not 1 <= a.nprobe <= K:
        raise SystemExit(f"search: --nprobe must be in [1, {K}], got {a.nprobe}")
    index, n = _search_index(a, km, comm)
    Q = np.load(a.queries, allow_pickle=False)
    lims, rows, dist = index.range_search(Q, a.radius, nprobe=a.nprobe, squared=a.squared)
    if comm.rank == 0:
        if a.output:
            np.savez(a.output, lims=lims.astype(np.int64), rows=rows.astype(np.int64),
                     distances=dist.astype(np.float32))
        print(json.dumps({"n_samples": n, "n_queries": int(lims.shape[0] - 1), "radius": float(a.radius),
                          "nprobe": int(a.nprobe), "found": int(rows.shape[0])}))
    comm.close()
    return 0


def cmd_blobs(a) -> int:
    from .data.blobs import make_blobs
    from .utils.io import save_points

    X, y = make_blobs(a.n, a.d, a.centers, std=a.std, seed=a.seed, return_labels=True)
    save_points(a.output, X)
    if a.labels:
        np.save(a.labels, y.numpy(), allow_pickle=False)
    print(json.dumps({"output": str(a.output), "shape": list(X.shape)}))
    return 0


def cmd_room(a) -> int:
    from .models.room import Room

    r = Room.from_json(Path(a.load).read_text(), a.room) if a.load else Room(a.room, seed=a.seed)
    if a.populate:
        r.populate_test_data()
    for name in a.centroid or []:
        r.add_centroid(name)
    if a.auto:
        r.auto_assign(seed=a.seed)
    if a.iteration is not None:
        r.set_iteration(a.iteration)
    if a.export:
        Path(a.export).write_text(r.export_json())
    if a.link is not None:
        print(r.share_link(a.link))
    if a.coin:
        print(r.coin())
    if a.d12:
        print(f"d12 \u2192 {r.d12()}")
    if a.shuffle_names:
        print("Suggested order:\n\n" + "\n".join(r.shuffled_titles()))
    d = r.dashboard()
    print("\n".join(d["chips"] + [" ".join(x for x in (row["name"], f"{row['bar_pct']}%", row["cohesion"],
                                                             row["top"], row["suggested"])) for row in d["rows"]]))
    return 0


def cmd_serve(a) -> int:
    """`mikmeans serve`: the room board and model serving over HTTP (mikmeans/serve.py)."""
    from .serve import serve

    session = None
    if a.found is not None or a.join:
        session = {"store_host": a.store_host, "store_port": a.store_port,
                   "found": a.found if a.found is not None else None, "member": a.member, "user": a.user}
    serve(a.room, a.model, host=a.host, port=a.port, device=a.device, session=session)
    return 0


def cmd_session(a) -> int:
    """A scripted participant of a live room session (parallel/elastic.py): ``--found ROOM``
    hosts the rendezvous store and starts the session, otherwise ``--join`` enters it; the
    edits given on the command line are submitted in the first round, every round prints one
    JSON status line, and all participants stop together at ``--until-round`` (the round
    counter is replicated)."""
    import datetime
    import os
    import socket
    import time

    import torch.distributed as dist

    from .parallel.elastic import ElasticRoomReplica

    store = dist.TCPStore(a.host, a.port, is_master=a.found is not None, wait_for_workers=False,
                          timeout=datetime.timedelta(seconds=a.timeout))
    member = a.member or f"{socket.gethostname()}-{os.getpid()}"
    kw = dict(user=a.user, seed=a.seed, timeout_s=a.timeout)
    if a.found is not None:
        state = Path(a.load).read_text() if a.load else None
        rep = ElasticRoomReplica.found(store, member, a.found or None, state_json=state, **kw)
    else:
        rep = ElasticRoomReplica.join(store, member, **kw)
    first = True
    while rep.round < a.until_round and not rep.left:
        if first:
            if a.populate:
                rep.populate_test_data()
            for name in a.centroid or []:
                rep.add_centroid(name)
            for spec in a.card or []:
                title, _, traits = spec.partition(":")
                rep.add_card(title, [t for t in traits.split(",") if t] or ["", ""])
            if a.auto:
                rep.auto_assign(seed=a.seed)
            first = False
        if a.leave_at is not None and rep.round >= a.leave_at:
            rep.leave()
        rep.sync()
        print(json.dumps({"member": member, "round": rep.round, "epoch": rep.epoch, "peers": rep.peers,
                          "roster": rep.roster, "left": rep.left, "digest": rep.digest()[:16]}), flush=True)
        time.sleep(a.interval)
    if a.export:
        Path(a.export).write_text(rep.room.export_json())
    return 0


def cmd_export(a) -> int:
    """Checkpoint -> flat-float centroid JSON, or a room-export JSON whose centroids
    are the model's clusters (named by their top features when a vocabulary exists)."""
    from .utils.checkpoint import load_checkpoint
    from .utils.jsjson import centroids_to_json

    ck = load_checkpoint(a.model)
    C = ck["centers"]
    if a.format == "flat":
        Path(a.output).write_text(centroids_to_json(C))
    else:
        from .models.room import Room

        r = Room(a.room or ck.get("config", {}).get("run_id"), seed_jessica=False, seed=0)
        vocab = ck.get("vocab")
        names = None
        if vocab:
            from .utils.traits import label_clusters

            names = label_clusters(C.numpy(), [1] * C.shape[0], vocab)
        r.max_centroids = max(r.max_centroids, C.shape[0])
        for k in range(C.shape[0]):
            r.add_centroid((names[k] if names and names[k] else None) or f"Centroid {k + 1}",
                           cid=f"c:{k}")
        r.set_iteration(int(ck["iteration"]))
        Path(a.output).write_text(r.export_json())
    print(json.dumps({"output": a.output, "format": a.format, "k": int(C.shape[0])}))
    return 0


def cmd_import(a) -> int:
    """Room-export JSON -> numeric model: cards become multi-hot trait vectors, the
    room's centroids seed k-means (auto_assign), the result is saved as a checkpoint."""
    from .models.room import Room
    from .utils.checkpoint import save_checkpoint
    from .utils.traits import encode_traits

    r = Room.from_json(Path(a.room).read_text())
    dash = r.auto_assign(seed=a.seed) if a.assign else r.dashboard()
    X, vocab = encode_traits(r.cards)
    cents = []
    for c in r.centroids:
        members = [i for i, card in enumerate(r.cards) if card.get("assignedTo") == c["id"]]
        cents.append(X[members].mean(0) if members else np.zeros(X.shape[1], dtype=np.float32))
    C = torch.from_numpy(np.stack(cents).astype(np.float32)) if cents else torch.zeros(0, X.shape[1])
    save_checkpoint(a.output, C, int(r.meta.get("iteration") or 0), {"run_id": r.room, "mode": r.meta.get("mode")},
                    extra={"vocab": vocab, "centroid_ids": [c["id"] for c in r.centroids],
                           "centroid_names": [c["name"] for c in r.centroids]})
    if a.save_room:
        Path(a.save_room).write_text(r.export_json())
    print("\n".join(dash["chips"]))
    return 0


def cmd_launch(a, rest) -> int:
    """``mikmeans launch --nproc N [--max-restarts R] -- <command> ...``: run a mikmeans
    command as an N-rank job (one process per GPU, RCCL) and restart it as a FRESH process
    tree when it fails; with ``--checkpoint-dir`` the restart resumes from the last
    checkpoint (``--resume auto`` is added).  This process never touches the GPU."""
    from .parallel.launch import launch_self

    if rest and rest[0] == "--":
        rest = rest[1:]
    if not rest:
        raise SystemExit("usage: mikmeans launch --nproc N [--max-restarts R] -- <command> [args]")
    if "--checkpoint-dir" in rest and "--resume" not in rest:
        rest = [*rest, "--resume", "auto"]
    return launch_self(a.nproc, ["-m", "mikmeans", *rest], max_restarts=a.max_restarts)


def cmd_bench(a, rest) -> int:
    root = Path(__file__).resolve().parent.parent
    sys.path.insert(0, str(root))
    import bench  # noqa: E402

    bench.main(rest)
    return 0


def cmd_plan(a) -> int:
    """HBM plan of a fit (parallel/memplan.py) for N rows over W ranks: resident or
    streamed, the chunk, every buffer's bytes.  Budget: --budget-gb, MIKMEANS_HBM_BYTES,
    this GPU's free memory, or else an idle MI355X (98 % of 288 GB)."""
    import os

    from .parallel import memplan, shard_sizes

    n_local = max(shard_sizes(a.n, a.world))
    if a.budget_gb:
        budget = int(a.budget_gb * 1e9)
    elif os.environ.get("MIKMEANS_HBM_BYTES") or torch.cuda.is_available():
        budget = memplan.hbm_budget()
    else:
        budget = int(memplan.HBM_BYTES * 0.98)
    try:
        if a.batch_size > 0:
            pl = memplan.plan_minibatch(n_local, a.d, a.k, a.dtype, batch_rows=a.batch_size, resident=True)
            pl.budget = budget
            if not pl.fits:
                pl = memplan.plan_minibatch(n_local, a.d, a.k, a.dtype, batch_rows=a.batch_size, resident=False)
                pl.budget = budget
        else:
            fkw = dict(budget=budget, x_on_device=False, incremental=not a.full_mstep, init=a.init)
            pl = None
            if a.algorithm == "auto":   # (KMeans' default: the bounds when they fit beside a resident shard)
                try:
                    pl = memplan.plan_fit(n_local, a.d, a.k, a.dtype, bounded=True, **fkw)
                    pl = pl if pl.mode == "resident" else None
                except memplan.HBMCapacityError:
                    pl = None
            if pl is None:
                pl = memplan.plan_fit(n_local, a.d, a.k, a.dtype, bounded=a.algorithm in ("hamerly", "elkan"),
                                      **fkw)
    except memplan.HBMCapacityError as e:
        print(json.dumps({"error": str(e)}))
        return 1
    out = pl.as_dict()
    out["summary"] = pl.summary()
    out["world"] = a.world
    print(json.dumps(out, indent=None if a.compact else 1))
    return 0


def cmd_info(a) -> int:
    from .ops import native

    info = {"torch": torch.__version__, "hip": getattr(torch.version, "hip", None),
            "gpu": torch.cuda.is_available(), "native": native.available(), "native_path": native.loaded_path()}
    if torch.cuda.is_available():
        p = torch.cuda.get_device_properties(0)
        info.update(device=p.name, arch=getattr(p, "gcnArchName", None), cus=p.multi_processor_count,
                    hbm_gb=round(p.total_memory / 1e9, 1), n_gpus=torch.cuda.device_count())
    print(json.dumps(info))
    return 0


def build_parser():
    from .config import KMeansConfig

    ap = argparse.ArgumentParser(prog="mikmeans", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("fit", help="fit k-means")
    src = f.add_mutually_exclusive_group(required=True)
    src.add_argument("--input", help=".npy / .safetensors / .csv point matrix")
    src.add_argument("--blobs", help="synthetic data N,D,CENTERS (generated on device, per rank)")
    f.add_argument("--output", help="checkpoint directory")
    f.add_argument("--save-labels", action="store_true")
    KMeansConfig.add_arguments(f)
    p = sub.add_parser("predict", help="assign points with a saved model")
    p.add_argument("--model", required=True)
    p.add_argument("--input", required=True)
    p.add_argument("--output")
    p.add_argument("--top", type=int, default=0, metavar="M",
                   help="write the M nearest centres of every row, nearest first ([n, M] labels)")
    p.add_argument("--distances-output", metavar="PATH", help="with --top: the [n, M] distances (.npy)")
    p.add_argument("--device")
    rp = sub.add_parser("report", help="per-cluster quality of a dataset under a saved model")
    rp.add_argument("--model", required=True)
    rp.add_argument("--input", required=True)
    rp.add_argument("--output", help="write the whole report here as JSON")
    rp.add_argument("--exemplars", type=int, default=0, metavar="M",
                    help="add every cluster's M rows nearest its centre (1..64) to the written report")
    rp.add_argument("--farthest", action="store_true", help="with --exemplars: the M farthest rows instead")
    rp.add_argument("--quantiles", metavar="Q,Q,...",
                    help="add every cluster's exact distance quantiles (1..8 values in [0, 1], e.g. 0.5,0.9,0.99) "
                         "to the written report")
    rp.add_argument("--device")
    sp = sub.add_parser("search", help="the rows of a dataset nearest each query, through a saved model's clusters")
    sp.add_argument("--model", required=True)
    sp.add_argument("--input", help="the rows to index (.npy / .safetensors / .csv)")
    sp.add_argument("--index", metavar="DIR", help="in place of --input: a saved index (mikmeans index) to load")
    sp.add_argument("--queries", required=True, help="the query rows (.npy)")
    sp.add_argument("--top", type=int, metavar="M", help="rows per query (1..32; 1..2048 with --deep)")
    sp.add_argument("--deep", action="store_true",
                    help="with --top: ClusterIndex.search_deep, the same result for up to 2048 rows per query")
    sp.add_argument("--radius", type=float, metavar="R",
                    help="in place of --top: every row within R of each query (with --squared, R is the squared "
                         "radius); writes lims, rows and distances")
    sp.add_argument("--nprobe", type=int, default=8, metavar="P",
                    help="clusters searched per query (1..n_clusters; n_clusters = exact search)")
    sp.add_argument("--refine", metavar="ROWS.npy",
                    help="with a PQ index: re-rank every probed list's shortlist on these rows (the ones the index was "
                         "built over; memory-mapped), PQIndex.search(refine=)")
    sp.add_argument("--shortlist", type=int, metavar="S",
                    help="with --refine: rows the codes keep of every probed list (1..32, or 64, 96, ..., 256; default 32)")
    sp.add_argument("--squared", action="store_true", help="write squared distances")
    sp.add_argument("--output", help="write rows and distances here (.npz)")
    sp.add_argument("--device")
    ip = sub.add_parser("index", help="build, update and save the index of a dataset under a saved model")
    ip.add_argument("--model", required=True)
    ip.add_argument("--output", required=True, metavar="DIR", help="the index directory (loaded first if it holds one "
                                                                    "and no --input is given)")
    ip.add_argument("--input", help="the rows to index (.npy / .safetensors / .csv)")
    ip.add_argument("--add", metavar="X2", help="rows to add to the index (.npy / .safetensors / .csv)")
    ip.add_argument("--remove", metavar="IDS", help="row ids to take out of the index (.npy, integers)")
    ip.add_argument("--pq", type=int, metavar="M", help="build a product-quantised index of M one-byte codes a row "
                                                        "(KMeans.build_pq_index; M in 8, 16, 32, 64) from --input")
    ip.add_argument("--train-rows", type=int, default=65536, help="with --pq: rows the codebooks are fitted on")
    ip.add_argument("--device")
    b = sub.add_parser("blobs", help="write a synthetic dataset")
    b.add_argument("--n", type=int, required=True)
    b.add_argument("--d", type=int, required=True)
    b.add_argument("--centers", type=int, required=True)
    b.add_argument("--std", type=float, default=1.0)
    b.add_argument("--seed", type=int, default=0)
    b.add_argument("--output", required=True)
    b.add_argument("--labels")
    r = sub.add_parser("room", help="headless trait-card room")
    r.add_argument("--room")
    r.add_argument("--load", help="import a room JSON export")
    r.add_argument("--populate", action="store_true", help="add the 11 test cards")
    r.add_argument("--centroid", action="append", help="add a centroid (repeatable, max 3)")
    r.add_argument("--auto", action="store_true", help="assign cards by numeric k-means")
    r.add_argument("--iteration", type=int)
    r.add_argument("--export", help="write kmeans-room JSON here")
    r.add_argument("--seed", type=int, default=0)
    r.add_argument("--link", nargs="?", const="", default=None, metavar="BASE_URL",
                   help="print the share link (?room=<code>)")
    r.add_argument("--coin", action="store_true", help="flip a coin (Heads/Tails)")
    r.add_argument("--d12", action="store_true", help="roll a twelve-sided die")
    r.add_argument("--shuffle-names", action="store_true", help="print a shuffled order of the card titles")
    sv = sub.add_parser("serve", help="HTTP service: the room board page + JSON API, and model serving")
    sv.add_argument("--room", default=None, help="room export JSON to start from")
    sv.add_argument("--model", default=None, help="fitted model directory (KMeans.save) to serve /api/predict")
    sv.add_argument("--host", default="127.0.0.1")
    sv.add_argument("--port", type=int, default=8000)
    sv.add_argument("--device", default=None)
    # serve one member of a live replicated room session (parallel/elastic.py)
    sg = sv.add_mutually_exclusive_group()
    sg.add_argument("--found", nargs="?", const="", metavar="ROOM",
                    help="start a live session (hosts its rendezvous store) and serve it")
    sg.add_argument("--join", action="store_true", help="join a running session and serve it")
    sv.add_argument("--store-host", default="127.0.0.1", help="session rendezvous (TCPStore) host")
    sv.add_argument("--store-port", type=int, default=29555, help="session rendezvous port")
    sv.add_argument("--member", help="unique member id (default host-pid)")
    sv.add_argument("--user", help="this member's display name")
    se = sub.add_parser("session", help="one participant of a live replicated room session")
    se.add_argument("--host", default="127.0.0.1", help="rendezvous (TCPStore) host")
    se.add_argument("--port", type=int, required=True)
    g = se.add_mutually_exclusive_group(required=True)
    g.add_argument("--found", nargs="?", const="", metavar="ROOM", help="start the session (hosts the store)")
    g.add_argument("--join", action="store_true", help="join a running session")
    se.add_argument("--member", help="unique member id (default host-pid)")
    se.add_argument("--user", help="display name (the reference's presence name)")
    se.add_argument("--load", help="--found: start from a room JSON export")
    se.add_argument("--populate", action="store_true")
    se.add_argument("--centroid", action="append")
    se.add_argument("--card", action="append", metavar="TITLE:TRAIT1,TRAIT2")
    se.add_argument("--auto", action="store_true")
    se.add_argument("--until-round", type=int, default=10)
    se.add_argument("--leave-at", type=int, help="leave once the session reaches this round")
    se.add_argument("--interval", type=float, default=0.1, help="seconds between rounds")
    se.add_argument("--seed", type=int, default=0)
    se.add_argument("--timeout", type=float, default=120.0)
    se.add_argument("--export", help="write the room JSON here at the end")
    e = sub.add_parser("export", help="checkpoint -> flat centroid JSON or room-export JSON")
    e.add_argument("--model", required=True)
    e.add_argument("--format", choices=["flat", "room"], default="flat")
    e.add_argument("--room", help="room code for --format room")
    e.add_argument("--output", required=True)
    i = sub.add_parser("import", help="room-export JSON -> numeric checkpoint (trait vectors)")
    i.add_argument("--room", required=True, help="kmeans-room-*.json")
    i.add_argument("--output", required=True, help="checkpoint directory")
    i.add_argument("--assign", action="store_true", help="re-assign cards by numeric k-means first")
    i.add_argument("--save-room", help="also write the (re-assigned) room JSON")
    i.add_argument("--seed", type=int, default=0)
    sub.add_parser("bench", help="headline benchmark (args forwarded to bench.py)", add_help=False)
    sub.add_parser("launch", help="N-rank job with restarts from the last checkpoint", add_help=False)
    sub.add_parser("info", help="environment / build info")
    pl = sub.add_parser("plan", help="HBM plan of a fit: resident / streamed, chunk rows, buffer bytes")
    pl.add_argument("--n", type=int, required=True, help="total rows (over all ranks)")
    pl.add_argument("--d", type=int, required=True)
    pl.add_argument("--k", type=int, required=True)
    pl.add_argument("--world", type=int, default=1)
    pl.add_argument("--dtype", default="bfloat16")
    pl.add_argument("--init", default="k-means++")
    pl.add_argument("--batch-size", type=int, default=0, help="> 0: plan a mini-batch fit")
    pl.add_argument("--full-mstep", action="store_true", help="no incremental M-step buffers")
    pl.add_argument("--algorithm", default="auto", choices=["auto", "lloyd", "hamerly", "elkan"],
                    help="hamerly: the bounded E-step's per-row bounds too; auto: them when they fit resident")
    pl.add_argument("--budget-gb", type=float, default=None)
    pl.add_argument("--compact", action="store_true")
    return ap


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    if argv and argv[0] == "bench":
        return cmd_bench(None, argv[1:])
    if argv and argv[0] == "launch":
        la = argparse.ArgumentParser(prog="mikmeans launch", description=cmd_launch.__doc__)
        la.add_argument("--nproc", type=int, default=1, help="ranks (one per GPU)")
        la.add_argument("--max-restarts", type=int, default=0, help="fresh-process restarts after a failure")
        a, rest = la.parse_known_args(argv[1:])
        return cmd_launch(a, rest)
    a = build_parser().parse_args(argv)
    return {"fit": cmd_fit, "predict": cmd_predict, "report": cmd_report, "search": cmd_search, "index": cmd_index, "blobs": cmd_blobs, "room": cmd_room, "session": cmd_session,
            "export": cmd_export, "import": cmd_import, "info": cmd_info, "plan": cmd_plan,
            "serve": cmd_serve}[a.cmd](a)


if __name__ == "__main__":
    sys.exit(main())
