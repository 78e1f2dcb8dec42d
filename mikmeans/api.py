"""Public estimator API: ``KMeans``, ``MiniBatchKMeans``, functional ``fit`` / ``predict``.

The surface follows scikit-learn's (``fit``, ``predict``, ``fit_predict``,
``transform``, ``score``, ``cluster_centers_``, ``labels_``, ``inertia_``,
``n_iter_``) on a PyTorch-ROCm engine: GPU tensors run the gfx950 kernels, CPU
tensors the PyTorch reference path, and a multi-process job (one rank per GPU,
RCCL) fits on per-rank shards with :class:`~mikmeans.parallel.Comm`.

Reference parity map: assignment of points to centroids
(R14/R25-R27 drag/drop + select, app.mjs:358-402) -> ``predict``/E-step;
centroid management (R13 addCentroid/removeCentroid, app.mjs:125-142) ->
``n_clusters``/``init``; locked centroids (app.mjs:128, :360) -> ``frozen``;
iteration counter + metric snapshots (R23/R31, app.mjs:288, :498-508) ->
``n_iter_`` / ``history_``; export/import (R21/R22) -> ``save``/``load`` and
:mod:`mikmeans.utils.io_json`.
"""
from __future__ import annotations

import dataclasses
import math
import time

import numpy as np
import torch

from .config import KMeansConfig, resolve_dtype
from .models.init import resolve_init
from .models.lloyd import LloydEngine, tol_to_abs
from .models.minibatch import MiniBatchEngine
from . import ops
from .ops import pad_columns
from .parallel.comm import Comm, get_comm
from .utils import faults
from .utils import metrics as mmetrics


def _default_device(device, X=None):
    """Explicit device > the input tensor's device > cuda when available > cpu."""
    if device is not None:
        return torch.device(device)
    if X is not None and torch.is_tensor(X):
        return X.device
    return torch.device("cuda" if torch.cuda.is_available() else "cpu")


def _to_tensor(X, device, dtype):
    was_numpy = not torch.is_tensor(X)
    t = torch.as_tensor(np.asarray(X) if was_numpy else X)
    if t.dim() != 2:
        raise ValueError(f"X must be 2-D [n_samples, n_features], got shape {tuple(t.shape)}")
    t = t.to(device=device)
    if t.dtype != dtype:
        t = t.to(dtype)
    return t, was_numpy


def _unit_rows(X: torch.Tensor, block: int = 1 << 22) -> torch.Tensor:
    """Rows scaled to unit L2 norm (f32 arithmetic, result in X's dtype; zero rows stay 0)."""
    out = torch.empty_like(X)
    for i in range(0, X.shape[0], block):
        xb = X[i : i + block].to(torch.float32)
        out[i : i + block] = (xb / xb.norm(dim=1, keepdim=True).clamp_min(1e-30)).to(X.dtype)
    return out


def native_dpad(D: int, dtype) -> int:
    """The MFMA kernels' padded width for D features (0: D > 1024, PyTorch GEMM path)."""
    from .ops import native

    return native.dpad_for(pad_columns(torch.empty((0, D), dtype=dtype)).shape[1], dtype)


def native_mod():
    from .ops import native

    return native.require()


def _device_rows(X: torch.Tensor, device, dtype, gpu: bool, block_bytes: int = 1 << 26) -> torch.Tensor:
    """``X`` on ``device`` in ``dtype`` -- column-padded to 16-byte rows for the GPU kernels --
    built block by block: a host block lands on the device in its own dtype (≤ 64 MB,
    memplan.staging_items) and is converted there, so no full-size temporary in another
    dtype ever exists.  ``X`` itself when it already qualifies."""
    if not gpu:
        t = X.to(device=device)
        return t if t.dtype == dtype else t.to(dtype)
    if X.device == device and X.dtype == dtype:
        P = pad_columns(X)
        if P is X:
            return X
    n, D = X.shape
    v = 8 if dtype == torch.bfloat16 else 4
    Dp = -(-D // v) * v
    out = torch.empty((n, Dp), dtype=dtype, device=device)
    if Dp > D:
        out[:, D:].zero_()
    rows = max(1, block_bytes // max(1, D * max(X.element_size(), out.element_size())))
    for i in range(0, n, rows):
        blk = X[i : i + rows]
        if blk.device != out.device:
            blk = blk.to(out.device)          # the staging block, in the source dtype
        out[i : i + rows, :D].copy_(blk)      # cast (and pad) on the device
        del blk
    return out


def buf_empty(eng, device) -> torch.Tensor:
    """A 0-row batch for a rank with an empty shard (it still joins every step's all-reduce)."""
    return torch.zeros((0, eng.Dp), dtype=eng.dtype, device=device)


def _shard_info(n_local: int, comm: Comm, device):
    sizes = comm.all_gather(torch.tensor([n_local], dtype=torch.int64, device=device)).reshape(-1).cpu()
    start = int(sizes[: comm.rank].sum())
    return int(sizes.sum()), start


def _allreduce(comm):
    """The in-place sum over the ranks of ``comm``, or None where there is nothing to sum over."""
    return comm.allreduce_ if comm is not None and comm.grouped else None


def _jsonable(v):
    """Plain JSON values: lists for arrays, None for NaN, "Infinity" for an infinite float."""
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    if torch.is_tensor(v) or isinstance(v, np.ndarray):
        v = v.tolist()
    if isinstance(v, (list, tuple)):
        return [_jsonable(x) for x in v]
    if isinstance(v, float) and not math.isfinite(v):
        return None if math.isnan(v) else ("Infinity" if v > 0 else "-Infinity")
    return v


@dataclasses.dataclass(eq=False)
class ClusterReport:
    """Per-cluster quality of a data set under fitted centres (``cluster_report``).

    Per cluster, ``[K]`` (tensors on the model's device, NumPy arrays for NumPy input):
    ``counts`` (rows with a finite distance), ``cluster_inertia`` (sum of squared distances),
    ``mean_distance``, ``rms_distance``, ``radius`` (the largest distance),
    ``cluster_silhouette`` (mean simplified silhouette 1 - a / b: a the distance to the own,
    b to the second-nearest centre) and ``n_nonfinite`` (rows left out because their distance
    is NaN or infinite).  Empty clusters have NaN means and radius 0.  Totals: ``n_samples``,
    ``inertia``, ``silhouette`` (NaN for one cluster), ``davies_bouldin`` (on the mean
    distances and the centre separations; NaN with fewer than two non-empty clusters) and
    ``balance`` ({max, min, gap, ratio} of the counts).  ``table`` is the int64
    ``[K, QUALITY_WORDS]`` reduction everything was decoded from (csrc/quality.hip)."""

    counts: object
    cluster_inertia: object
    mean_distance: object
    rms_distance: object
    radius: object
    cluster_silhouette: object
    n_nonfinite: object
    n_samples: int
    inertia: float
    silhouette: float
    davies_bouldin: float
    balance: dict
    table: object

    PER_CLUSTER = ("counts", "cluster_inertia", "mean_distance", "rms_distance", "radius", "cluster_silhouette",
                   "n_nonfinite")

    @classmethod
    def from_table(cls, table: torch.Tensor, centers: torch.Tensor, dtype):
        rep = ops.quality_decode(table, centers, dtype)
        for k in cls.PER_CLUSTER:
            rep[k] = rep[k].to(table.device)
        return cls(table=table, **rep)

    def numpy(self) -> "ClusterReport":
        """The same report with NumPy arrays."""
        return dataclasses.replace(self, table=self.table.cpu().numpy(),
                                   **{k: getattr(self, k).cpu().numpy() for k in self.PER_CLUSTER})

    def to_dict(self) -> dict:
        """Plain lists, ints and floats (NaN as None, an infinite ratio as "Infinity")."""
        out = {k: getattr(self, k) for k in ("n_samples", "inertia", "silhouette", "davies_bouldin", "balance")}
        out["n_clusters"] = len(self.counts)
        out["n_nonfinite"] = int(self.n_nonfinite.sum())
        out["clusters"] = {k: getattr(self, k) for k in self.PER_CLUSTER}
        return _jsonable(out)


def _report_table(centers, comm, dtype, fold) -> ClusterReport:
    """``fold(table)`` accumulates this rank's rows; the table is then summed (its maximum
    word maximised) over the ranks of ``comm`` and decoded, the same on every rank."""
    table = torch.zeros((centers.shape[0], ops.QUALITY_WORDS), dtype=torch.int64, device=centers.device)
    fold(table)
    reduce = _allreduce(comm)
    if reduce is not None:
        mx = table[:, 17].clone()
        reduce(table)
        comm.allreduce_max_(mx)
        table[:, 17] = mx
    return ClusterReport.from_table(table, centers, dtype)


def _merge_rank_lists(hi: torch.Tensor, rows: torch.Tensor, comm):
    """Every rank's ``[L, m]`` lists of (key word, global row) pairs -- row -1 an empty slot -- merged
    over the ranks of ``comm``: all-gathered, the m lexicographically smallest pairs kept per list.
    ``(hi, rows)``, the same on every rank."""
    L, m = rows.shape
    last = 1 << 62                                            # (past every key word: they are below 2^31)
    hi = torch.where(rows < 0, last, hi)
    W = comm.world
    hi = comm.all_gather(hi).permute(1, 0, 2).reshape(L, W * m)
    rows = comm.all_gather(rows).permute(1, 0, 2).reshape(L, W * m)
    o = torch.argsort(rows, dim=1, stable=True)               # by the global row, then (stable) by the key
    hi, rows = hi.gather(1, o), rows.gather(1, o)             # word: the pairs in lexicographic order
    o = torch.argsort(hi, dim=1, stable=True)[:, :m]
    return hi.gather(1, o), rows.gather(1, o)


def _exemplar_lists(K: int, m: int, device, comm, n_local: int, farthest: bool, squared: bool, fold):
    """``fold(table)`` min-inserts this rank's rows (indexed from 0) into an empty exemplar
    table; the lists are then merged over the ranks of ``comm`` -- every rank's ``[K, m]``
    (key word, global row) pairs all-gathered, the m lexicographically smallest kept per
    cluster -- and decoded: ``(rows int64 [K, m], distances float32 [K, m])``, the same on every
    rank and bit for bit the one-rank result on the concatenated shards."""
    if int(n_local) >= 1 << 32:
        raise ValueError(f"cluster_exemplars takes fewer than 2^32 rows in one call, got {int(n_local)}")
    table = ops.exemplar_new(K, m, device)
    fold(table)
    if _allreduce(comm) is not None:
        _, start = _shard_info(int(n_local), comm, device)
        rows, _ = ops.exemplar_decode(table, row_start=start)
        hi, rows = _merge_rank_lists(table >> 32, rows, comm)
        bits = torch.where(rows < 0, 0, (0x7F7FFFFF - hi) if farthest else hi)
        d2 = torch.where(rows < 0, float("nan"), bits.to(torch.int32).view(torch.float32))
    else:
        rows, d2 = ops.exemplar_decode(table, farthest=farthest)
    return rows, (d2 if squared else d2.sqrt())


def _merge_search_keys(keys: torch.Tensor, comm, row_start: int):
    """This rank's sorted search keys ``[nq, m]`` decoded and merged over the ranks of ``comm``
    (:func:`_merge_rank_lists`): ``(rows int64 [nq, m], d2 float32 [nq, m])``, the same on every rank."""
    rows, d2 = ops.index_decode(keys, row_start=row_start)
    if _allreduce(comm) is None:
        return rows, d2
    hi, rows = _merge_rank_lists(keys >> 32, rows, comm)
    d2 = torch.where(rows < 0, float("nan"), torch.where(rows < 0, 0, hi).to(torch.int32).view(torch.float32))
    return rows, d2


class ClusterIndex:
    """The rows of a dataset grouped by their nearest centre (an inverted-file index over the fitted
    clusters), from :meth:`KMeans.build_index`.  ``n_rows``: the rows given (this rank's shard);
    ``list_sizes`` (int64 [K]) and ``offsets`` (int64 [K + 1]): every list's length and where it
    starts in ``order``; ``order``: the row ids, list after list and ascending within a list (rows
    whose distance to their centre is not finite are in no list); ``nbytes``: what the index keeps
    on its device.  In a multi-rank job the lists hold the rank's shard under global row ids.

    The index can change and be kept (one-rank jobs): :meth:`add` and :meth:`remove` give rows to and
    take rows from the lists, :meth:`save` and :meth:`load` keep it on disk.  Row ids are handed out
    in arrival order and never reused: ``n_rows`` counts the ids handed out (the rows of the build and
    every row added since), ``n_indexed`` the rows in a list now."""

    FORMAT = "mikmeans-index-v1"
    TENSORS = "index.safetensors"
    META = "index.json"

    def __init__(self, model, index, row_start: int, comm):
        self._model, self._index, self.row_start, self._comm = model, index, int(row_start), comm

    @property
    def n_rows(self) -> int:
        return int(self._index.n)

    @property
    def n_indexed(self) -> int:
        return int(self._index.offsets[-1])

    def _one_rank(self, what: str):
        if _allreduce(self._comm) is not None:
            raise NotImplementedError(f"ClusterIndex.{what} is not available in a multi-rank job")

    def _check_plan(self, what: str, n_total: int, block_rows=None):
        """The update's memory plan against the HBM budget (GPU indexes), before anything is allocated."""
        ix = self._index
        if not ix.pack.is_cuda:
            return
        from .parallel import memplan

        D = int(self._model.cluster_centers_.shape[1])
        plan = memplan.plan_index_update(ix.n, n_total, D, ix.K, ix.dtype, block_rows=block_rows)
        plan.budget = memplan.hbm_budget(ix.pack.device)
        if not plan.fits:
            raise memplan.HBMCapacityError(f"{what}: {plan.summary()} does not fit")

    def add(self, X, *, block_rows: int | None = None) -> int:
        """Add the rows of ``X`` to the lists of their nearest centres: returns the first (global)
        row id of the batch, whose rows take consecutive ids.  A row's list follows the rule of
        :meth:`KMeans.build_index` (cosine models index unit rows; a row whose distance to its centre
        is NaN or infinite takes an id and is in no list), and the index afterwards equals, tensor for
        tensor, the one built over all its rows at once.  Only the new rows meet the centres: the
        rows already held are copied from the old row pack into the new one (csrc/ivf.hip: the
        repack), so the old and the new index are both alive for a moment
        (``memplan.plan_index_update``, checked against the HBM budget up front).  numpy or torch,
        host or device rows (host rows bound for a GPU index cross in blocks of ``block_rows``).
        After an exception the index is what it was."""
        self._one_rank("add")
        mdl, ix = self._model, self._index
        c = mdl.cluster_centers_
        if getattr(X, "ndim", 0) != 2 or int(X.shape[1]) != int(c.shape[1]):
            raise ValueError(f"add takes rows [n, {int(c.shape[1])}], got shape {tuple(getattr(X, 'shape', ()))}")
        n1 = int(X.shape[0])
        if ix.n + n1 >= 1 << 32:
            raise ValueError(f"an index takes fewer than 2^32 row ids, got {ix.n} + {n1}")
        self._check_plan("add", ix.n + n1, block_rows)
        new = ops.index_add(ix, None, c, block_rows=block_rows, n=n1, blocks=lambda: mdl._host_blocks(X, block_rows))
        self._index = new
        return self.row_start + ix.n

    def remove(self, ids) -> int:
        """Take the rows ``ids`` (global row ids, integers, in any order) out of their lists:
        returns how many left one (the one host read).  Duplicates, ids out of range, ids in no
        list and ids removed before are ignored; the rows that stay keep their ids and their
        order, and an id is never handed out again.  The index afterwards equals the one built
        over the rows that stay.  After an exception the index is what it was."""
        self._one_rank("remove")
        ix = self._index
        t = ids if torch.is_tensor(ids) else torch.as_tensor(np.asarray(ids))
        if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"remove takes integer row ids, got {t.dtype}")
        self._check_plan("remove", ix.n)
        new, removed = ops.index_remove(ix, t.reshape(-1).to(device=ix.order.device, dtype=torch.int64) - self.row_start)
        removed = int(removed)
        self._index = new
        return removed

    def save(self, path):
        """Write the index to the directory ``path``: ``index.safetensors`` (its tensors and the
        centres its rows were listed under) and ``index.json`` (the format version and ``n``, ``K``,
        ``D``, ``dtype``, ``native``, ``cols``, ``row_start``)."""
        import json
        import os
        from pathlib import Path

        from safetensors.torch import save_file

        self._one_rank("save")
        ix = self._index
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        blobs = {k: v.detach().to("cpu").contiguous() for k, v in ix.tensors().items()}
        blobs["centers"] = self._model.cluster_centers_.detach().to("cpu").contiguous()
        tmp = path / (self.TENSORS + ".tmp")
        save_file(blobs, str(tmp))
        os.replace(tmp, path / self.TENSORS)
        meta = {"format": self.FORMAT, "n": int(ix.n), "K": int(ix.K), "D": int(ix.D),
                "dtype": "bfloat16" if ix.dtype == torch.bfloat16 else "float32", "native": bool(ix.native),
                "cols": int(ix.cols), "row_start": int(self.row_start)}
        tmpm = path / (self.META + ".tmp")
        tmpm.write_text(json.dumps(meta))
        os.replace(tmpm, path / self.META)
        return path

    @classmethod
    def saved_at(cls, path) -> bool:
        """Whether the directory ``path`` holds a saved index."""
        from pathlib import Path

        return (Path(path) / cls.META).is_file() and (Path(path) / cls.TENSORS).is_file()

    @classmethod
    def load(cls, path, model, device=None) -> "ClusterIndex":
        """The index :meth:`save` wrote, for ``model`` (whose fitted centres must be the saved ones,
        bit for bit, and whose dtype and feature count the index's) on ``device`` (default: the
        model's).  It searches bit for bit as the saved one.  A fragment-packed (GPU) index loads to
        a GPU only and a natural-layout one to the CPU only, unless its rows are wider than the
        kernels."""
        import json
        from pathlib import Path

        from safetensors.torch import load_file

        model._check_fitted()
        comm = getattr(model, "comm", None) or get_comm()
        if _allreduce(comm) is not None:
            raise NotImplementedError("ClusterIndex.load is not available in a multi-rank job")
        path = Path(path)
        meta = json.loads((path / cls.META).read_text())
        if meta.get("format") != cls.FORMAT:
            raise ValueError(f"{path}: not a {cls.FORMAT} index (format {meta.get('format')!r})")
        c = model.cluster_centers_
        dev = torch.device(device) if device is not None else c.device
        ts = load_file(str(path / cls.TENSORS))
        saved_c = ts.pop("centers")
        dtype = torch.bfloat16 if meta["dtype"] == "bfloat16" else torch.float32
        if dtype != model.dtype:
            raise ValueError(f"the index holds {dtype} rows, the model's dtype is {model.dtype}")
        if saved_c.shape != c.shape or not torch.equal(saved_c, c.detach().to("cpu")):
            raise ValueError("the model's cluster_centers_ are not the centres the index was saved under")
        # what an index built for this model on dev has: stored columns, layout, pack columns
        F = int(c.shape[1])
        if dev.type == "cuda":
            D = int(pad_columns(torch.empty((0, F), dtype=dtype)).shape[1])
            dpad = native_dpad(F, dtype)
        else:
            D, dpad = F, 0
        if bool(meta["native"]) != bool(dpad):
            raise ValueError("a fragment-packed (GPU) index cannot be loaded to the CPU" if meta["native"] else
                             "a natural-layout (CPU) index cannot be loaded to a GPU")
        if (int(meta["K"]), int(meta["D"]), int(meta["cols"])) != (int(c.shape[0]), D, dpad or D):
            raise ValueError(f"the index holds {meta['K']} lists of {meta['D']}-feature rows, the model has "
                             f"{int(c.shape[0])} centres of {F} features")
        if dev.type != c.device.type:
            raise ValueError(f"the index would load to {dev}, the model's centres are on {c.device}")
        ts = {k: v.to(dev) for k, v in ts.items()}
        index = ops.RowIndex(int(meta["n"]), int(meta["K"]), int(meta["D"]), dtype, bool(meta["native"]),
                             int(meta["cols"]), ts["row_pack"], ts["cn"], ts["order"], ts["offsets"], ts["tile_offsets"])
        return cls(model, index, int(meta["row_start"]), comm)

    @property
    def offsets(self) -> torch.Tensor:
        return self._index.offsets

    @property
    def list_sizes(self) -> torch.Tensor:
        return self._index.offsets[1:] - self._index.offsets[:-1]

    @property
    def order(self) -> torch.Tensor:
        return self._index.order[: int(self._index.offsets[-1])] + self.row_start

    @property
    def nbytes(self) -> int:
        return self._index.nbytes

    def rows_of(self, k: int) -> torch.Tensor:
        """The row ids of cluster ``k``, ascending."""
        K = self._index.K
        if not 0 <= int(k) < K:
            raise ValueError(f"rows_of needs 0 <= k < n_clusters ({K}), got k = {k}")
        a, b = (int(v) for v in self._index.offsets[int(k) : int(k) + 2])
        return self._index.order[a:b] + self.row_start

    def search(self, Q, m: int, *, nprobe: int = 8, squared: bool = False):
        """The ``m`` indexed rows nearest every query among the lists of its ``nprobe`` nearest
        centres: ``(rows [nq, m] int64, distances [nq, m] float32)``, nearest first and equal
        distances by the lower row id; a query whose probed lists hold fewer than ``m`` rows is
        padded with row -1 and distance NaN.  ``1 <= m <= 32`` and ``1 <= nprobe <= n_clusters``;
        ``nprobe = n_clusters`` is the exact brute-force search over the indexed rows.  Distances
        are Euclidean as in :meth:`KMeans.transform` (``squared``: the kernel's squared values,
        bitwise ``ops.transform(Q, X.float(), squared=True)``'s; cosine models work on unit rows).

        On the GPU: the top-``nprobe`` kernel on the serving pack, a partition of the (query, probe)
        pairs by list and the scan kernel of csrc/ivf.hip, one wave per (list, block of queries
        probing it); a long list is not split over waves, so a single query runs one wave per
        probed list.  Results are bitwise the same from run to run.  In a multi-rank job ``Q`` is
        the same on every rank and every rank returns the one-rank result on the concatenated
        shards.  Queries with non-finite coordinates give unspecified results.  numpy in, numpy
        out; host queries bound for a GPU index go through in blocks."""
        mdl = self._model
        m = int(m)
        if not 1 <= m <= ops.INDEX_MAX_M:
            raise ValueError(f"search needs 1 <= m <= {ops.INDEX_MAX_M}, got m = {m}")
        c, nprobe = self._probe_args("search", Q, nprobe)
        (keys,), was_numpy = mdl._row_blocks(
            Q, lambda Qt, pk: (ops.index_search(self._index, Qt, c, m, nprobe, pack=pk),))
        rows, d2 = _merge_search_keys(keys, self._comm, self.row_start)
        d = d2 if squared else d2.sqrt()
        return (rows.cpu().numpy(), d.cpu().numpy()) if was_numpy else (rows, d)

    def search_deep(self, Q, m: int, *, nprobe: int = 8, squared: bool = False, passes: int | None = None):
        """:meth:`search` for up to ``ops.INDEX_DEEP_MAX_M`` = 2048 rows a query: ``(rows [nq, m] int64,
        distances [nq, m] float32)``, what :meth:`search` would return if its list were that long --
        the first ``m`` of the ascending ``(d2 bits << 32 | row)`` keys over the rows of the query's
        ``nprobe`` probed lists, equal distances by the lower row id, missing slots row -1 and
        distance NaN -- and for ``m <= 32`` :meth:`search`'s result bit for bit.  ``nprobe``,
        ``squared``, cosine models, numpy queries, host blocks and multi-rank jobs as in
        :meth:`search`.

        On the GPU no candidate list is kept: a radix select over the bits of the squared distances
        (csrc/deep.hip: per 8-bit digit one histogram pass over the walk of :meth:`search` and one
        select) finds a radius that is at least every query's m-th distance, and the two passes of
        :meth:`range_search` collect the rows under it, which are sorted and cut to ``m``.  The
        select stops as soon as the radius lets through at most ``ops.INDEX_DEEP_OVERSHOOT`` times
        the rows wanted (one scalar host read a pass, one more for the fill); ``passes`` = 1..4
        forces the pass count and does not change the result.  Rows tied with the m-th one are all
        under the exact radius, so ties there make the rows collected exceed ``m`` by the number
        of tied rows: inherent to the method, and the lower row ids are kept.  The memory plan
        (``memplan.plan_index_search_deep``) is checked against the HBM budget up front.  Queries
        with non-finite coordinates give unspecified results; the other queries' are unchanged."""
        mdl, ix = self._model, self._index
        m = int(m)
        if not 1 <= m <= ops.INDEX_DEEP_MAX_M:
            raise ValueError(f"search_deep needs 1 <= m <= {ops.INDEX_DEEP_MAX_M}, got m = {m}")
        if passes is not None and not 1 <= int(passes) <= 4:
            raise ValueError(f"search_deep needs passes in 1..4 (or None), got {passes}")
        c, nprobe = self._probe_args("search_deep", Q, nprobe)
        if ix.pack.is_cuda:
            from .parallel import memplan

            plan = memplan.plan_index_search_deep(ix.n, int(c.shape[1]), ix.K, ix.dtype, nq=int(Q.shape[0]), m=m,
                                                  nprobe=nprobe)
            plan.budget = memplan.hbm_budget(ix.pack.device) + sum(
                plan.persistent[k] for k in ("row_pack", "cn", "order", "offsets", "tile_offsets"))   # (held already)
            if not plan.fits:
                raise memplan.HBMCapacityError(f"search_deep: {plan.summary()} does not fit")
        (keys,), was_numpy = mdl._row_blocks(
            Q, lambda Qt, pk: (ops.index_search_deep(ix, Qt, c, m, nprobe, pack=pk, passes=passes),))
        rows, d2 = _merge_search_keys(keys, self._comm, self.row_start)
        d = d2 if squared else d2.sqrt()
        return (rows.cpu().numpy(), d.cpu().numpy()) if was_numpy else (rows, d)

    def _probe_args(self, what, Q, nprobe):
        """``(centres, nprobe)`` of a ``what`` ("search" / "range_search") over 2-D queries, checked."""
        c = self._model.cluster_centers_
        K, nprobe = int(c.shape[0]), int(nprobe)
        if not 1 <= nprobe <= K:
            raise ValueError(f"{what} needs 1 <= nprobe <= n_clusters ({K}), got nprobe = {nprobe}")
        if getattr(Q, "ndim", 2) != 2:
            raise ValueError(f"Q must be 2-D [n_queries, n_features], got shape {tuple(Q.shape)}")
        return c, nprobe

    def _range_args(self, Q, radius, nprobe, squared):
        """The checked arguments of a range search: ``(centres, nprobe, r2 float32 [nq] on the CPU)``."""
        c, nprobe = self._probe_args("range_search", Q, nprobe)
        nq = int(Q.shape[0])
        r = (radius.detach().cpu() if torch.is_tensor(radius) else torch.as_tensor(np.asarray(radius, dtype=np.float64)))
        if r.dim() > 1 or (r.dim() == 1 and r.shape[0] != nq):
            raise ValueError(f"radius must be a scalar or one value per query ({nq}), got shape {tuple(r.shape)}")
        if not bool((torch.isfinite(r) & (r >= 0)).all()):
            raise ValueError("radius must be finite and non-negative")
        r = r.to(torch.float32)
        r2 = r if squared else r * r
        if not bool(torch.isfinite(r2).all()):
            raise ValueError("radius squared must be finite in float32")
        return c, nprobe, r2.expand(nq).contiguous()

    def _range_blocks(self, Q, c, r2, nprobe, **kw):
        """``ops.index_range`` over the host blocks of ``Q``: a list of per-block results."""
        dev = c.device
        return [ops.index_range(self._index, Qt, c, r2[i : i + Qt.shape[0]].to(dev), nprobe, pack=pk, **kw)
                for i, Qt, pk in self._model._host_blocks(Q)]

    def range_count(self, Q, radius, nprobe: int = 8, squared: bool = False):
        """How many hits :meth:`range_search` gives every query: int64 ``[nq]``, equal to its
        ``lims[1:] - lims[:-1]``.  Only the count pass runs: nothing is allocated per hit and no
        host read is made; in a multi-rank job the ranks' counts are summed by one all-reduce."""
        c, nprobe, r2 = self._range_args(Q, radius, nprobe, squared)
        counts = torch.cat(self._range_blocks(Q, c, r2, nprobe, count_only=True))
        if _allreduce(self._comm) is not None:
            self._comm.allreduce_(counts)
        return counts if torch.is_tensor(Q) else counts.cpu().numpy()

    def range_search(self, Q, radius, nprobe: int = 8, squared: bool = False, sort: bool = True,
                     max_results: int | None = None):
        """Every indexed row within ``radius`` of each query, among the lists of the query's
        ``nprobe`` nearest centres: ``(lims int64 [nq + 1], rows int64 [total], distances float32
        [total])``, query q's hits ``rows[lims[q]:lims[q + 1]]`` (global row ids) and their distances.

        ``radius``: a non-negative finite scalar, or one value per query.  The test is made on
        squared values: a row is a hit where the kernel's float32 squared distance ``d2`` -- bitwise
        ``ops.transform(Q, X.float(), squared=True)``'s, as in :meth:`search` -- has ``d2 <= r2``,
        ``r2 = float32(radius) * float32(radius)`` rounded to float32 (``squared``: ``radius`` is
        ``r2`` itself and the distances returned are ``d2``; otherwise ``d2.sqrt()``).  ``r2`` must be
        finite.  A query with a NaN or infinite coordinate has no hits, rows in no list are never
        hits, and ``nprobe = n_clusters`` is the exact range search over the indexed rows.
        ``sort``: a query's hits nearest first, equal distances by the lower row id (the order of
        :meth:`search`); otherwise probe after probe (nearest centre first) and ascending row id
        within a probe, without a per-query sort.  Both orders are bitwise the same from run to
        run.  ``max_results``: raise ``ValueError`` if the total number of hits exceeds it, after a
        count pass of its own and before anything sized by the total is allocated.

        On the GPU (csrc/range.hip): the scan's work items -- one wave per (list, block of queries
        probing it); a long list is not split over waves -- in two passes, a count per (query, probe)
        pair and, after a cumulative sum, the fill.  The length of the result is only known after
        the count, so every block of queries costs one host read of its total; that is inherent to a
        variable-length result.  In a multi-rank job ``Q`` is the same on every rank and every rank
        returns the one-rank result on the concatenated shards (the ranks' hits are all-gathered
        and put in the same order).  numpy in, numpy out; host queries bound for a GPU index go
        through in blocks."""
        c, nprobe, r2 = self._range_args(Q, radius, nprobe, squared)
        grouped = _allreduce(self._comm) is not None
        nq, dev = int(Q.shape[0]), c.device
        if max_results is not None:
            counts = torch.cat(self._range_blocks(Q, c, r2, nprobe, count_only=True))
            if grouped:
                self._comm.allreduce_(counts)
            total = int(counts.sum())
            if total > int(max_results):
                raise ValueError(f"range_search found {total} rows, more than max_results = {int(max_results)}")
        parts = self._range_blocks(Q, c, r2, nprobe, sort=sort and not grouped, want_probe=grouped)
        counts = torch.cat([p[0][1:] - p[0][:-1] for p in parts])
        keys = torch.cat([p[1] for p in parts])
        rows = (keys & 0xFFFFFFFF) + self.row_start
        bits = keys >> 32
        if grouped:
            comm = self._comm
            qid = torch.repeat_interleave(torch.arange(nq, device=dev), counts, output_size=keys.numel())
            mine = torch.stack([qid, torch.cat([p[2] for p in parts]), bits, rows])
            sizes = comm.all_gather(torch.tensor([keys.numel()], dtype=torch.int64, device=dev)).reshape(-1).tolist()
            buf = torch.zeros((4, max(max(sizes), 1)), dtype=torch.int64, device=dev)
            buf[:, : keys.numel()] = mine
            every = comm.all_gather(buf)
            qid, probe, bits, rows = torch.cat([every[w, :, :s] for w, s in enumerate(sizes)], dim=1)
            comm.allreduce_(counts)
            o = torch.argsort(rows, stable=True)                      # by (query, bits | probe rank, row):
            o = o[torch.argsort((bits if sort else probe)[o], stable=True)]   # stable sorts, last key first
            o = o[torch.argsort(qid[o], stable=True)]
            bits, rows = bits[o], rows[o]
        lims = torch.zeros(nq + 1, dtype=torch.int64, device=dev)
        lims[1:] = torch.cumsum(counts, 0)
        d2 = bits.to(torch.int32).view(torch.float32)
        d = d2 if squared else d2.sqrt()
        if torch.is_tensor(Q):
            return lims, rows, d
        return lims.cpu().numpy(), rows.cpu().numpy(), d.cpu().numpy()


class PQIndex:
    """The rows of a dataset grouped by their nearest centre and kept as product-quantiser codes
    (IVF-PQ), from :meth:`KMeans.build_pq_index`: ``n_subvectors`` bytes a row instead of the row.
    ``n_rows``: the rows given; ``n_indexed``: the rows in a list; ``list_sizes`` / ``offsets`` /
    ``order`` / ``rows_of`` as in :class:`ClusterIndex`; ``codebooks`` float32 ``[n_subvectors, 256,
    dsub]``; ``nbytes``: what the index keeps on its device, ``n M + 8 n + 8 (K + 1) + 4 M 256 dsub``.
    One-rank jobs only; docs/PQ_INDEX.md has the definitions."""

    FORMAT = "mikmeans-pq-index-v1"
    TENSORS = "pq_index.safetensors"
    META = "pq_index.json"

    def __init__(self, model, index, row_start: int = 0):
        self._model, self._index, self.row_start = model, index, int(row_start)

    @property
    def n_rows(self) -> int:
        return int(self._index.n)

    @property
    def n_indexed(self) -> int:
        return int(self._index.offsets[-1])

    @property
    def n_subvectors(self) -> int:
        return int(self._index.M)

    @property
    def offsets(self) -> torch.Tensor:
        return self._index.offsets

    @property
    def list_sizes(self) -> torch.Tensor:
        return self._index.offsets[1:] - self._index.offsets[:-1]

    @property
    def order(self) -> torch.Tensor:
        return self._index.order[: int(self._index.offsets[-1])] + self.row_start

    @property
    def codebooks(self) -> torch.Tensor:
        return self._index.codebooks

    @property
    def nbytes(self) -> int:
        return self._index.nbytes

    def rows_of(self, k: int) -> torch.Tensor:
        """The row ids of cluster ``k``, ascending."""
        K = self._index.K
        if not 0 <= int(k) < K:
            raise ValueError(f"rows_of needs 0 <= k < n_clusters ({K}), got k = {k}")
        a, b = (int(v) for v in self._index.offsets[int(k) : int(k) + 2])
        return self._index.order[a:b] + self.row_start

    def _search_refined(self, Q, m: int, nprobe: int, squared: bool, refine, shortlist):
        """:meth:`search` with ``refine``: the shortlists of ``ops.pq_shortlist`` re-ranked on the rows."""
        mdl, ix = self._model, self._index
        if getattr(mdl, "metric", "euclidean") == "cosine":
            raise NotImplementedError("PQIndex.search(refine=) is not available for cosine models")
        ops.pq_shortlist_groups(32 if shortlist is None else shortlist)
        shortlist = 32 if shortlist is None else int(shortlist)
        c = mdl.cluster_centers_
        K, F, dev = int(c.shape[0]), int(c.shape[1]), ix.codes.device
        if torch.is_tensor(refine):
            X = refine
        else:
            import warnings

            with warnings.catch_warnings():     # (a read-only memory map: the rows are only ever read)
                warnings.simplefilter("ignore", UserWarning)
                X = torch.from_numpy(np.asarray(refine))
        if X.dim() != 2 or tuple(X.shape) != (ix.n, F):
            raise ValueError(f"refine takes the rows the index was built over, [{ix.n}, {F}], got shape {tuple(X.shape)}")
        if X.is_cuda and (X.dtype != ix.dtype or X.device != dev):
            raise ValueError(f"refine takes device rows of {ix.dtype} on {dev} (they are read in place), got "
                             f"{X.dtype} on {X.device}; pass them from the host or convert them")
        host = not X.is_cuda and ix.codes.is_cuda
        if not X.is_cuda and not host and X.dtype != ix.dtype:
            X = X.to(ix.dtype)
        if ix.codes.is_cuda:
            from .parallel import memplan

            plan = memplan.plan_pq_refine(ix.n, F, K, ix.M, ix.dtype, nq=int(Q.shape[0]), m=m, nprobe=nprobe,
                                          shortlist=shortlist, host_rows=host)
            plan.budget = memplan.hbm_budget(dev) + sum(
                plan.persistent[k] for k in ("codes", "order", "offsets", "codebooks"))   # (held already)
            if not plan.fits:
                raise memplan.HBMCapacityError(f"search: {plan.summary()} does not fit")
        (keys,), was_numpy = mdl._row_blocks(
            Q, lambda Qt, pk: (ops.pq_refine(ix, Qt, c, X, m, nprobe, shortlist, pack=pk),))
        rows, d2 = ops.index_decode(keys, row_start=self.row_start)
        d = d2 if squared else d2.sqrt()
        return (rows.cpu().numpy(), d.cpu().numpy()) if was_numpy else (rows, d)

    def search(self, Q, m: int, *, nprobe: int = 8, squared: bool = False, refine=None, shortlist=None):
        """The ``m`` indexed rows of least asymmetric distance to every query among the lists of its
        ``nprobe`` nearest centres: ``(rows [nq, m] int64, distances [nq, m] float32)``, nearest first
        and equal distances by the lower row id; padding is row -1 and distance NaN.  ``1 <= m <= 32``
        and ``1 <= nprobe <= n_clusters``.  A distance is the sum of ``n_subvectors`` table entries
        (``ops.pq_search``; ``squared``: that sum, otherwise its square root), an estimate of the
        distance to the row itself.  On the GPU: the top-``nprobe`` kernel, the transform kernel for
        the tables and the scan of csrc/pq.hip, one workgroup per (query, probed list, split) with the
        table in LDS; the memory plan (``memplan.plan_pq_search``) is checked against the HBM budget up
        front.  Results are bitwise the same from run to run.  numpy in, numpy out.

        ``refine=X`` re-ranks on the rows themselves: ``X`` ``[n_rows, n_features]`` (numpy or torch, host
        or device) holds the rows the index was built over, the codes pick ``shortlist`` rows of every
        probed list (``ops.pq_shortlist``: 1..32, or 64, 96, ..., 256; default 32) and the result is the
        ``m`` of them of least exact distance -- ``ops.rerank``'s float32 sum of squared differences
        (``squared``), or its square root -- equal distances by the lower row id.  Device rows must be in
        the model's dtype on the index's device and are read in place (csrc/rerank.hip).  Host rows
        of a GPU index cost one host read per block of queries: the block's candidate ids go to the
        host, the distinct rows are gathered there, cross to the device once in the model's dtype and
        meet the same kernel, so the result is bit for bit the one with device rows.  The memory plan
        is ``memplan.plan_pq_refine``.  Cosine models raise ``NotImplementedError``; ``shortlist``
        without ``refine`` is a ``ValueError``."""
        mdl, ix = self._model, self._index
        m = int(m)
        if not 1 <= m <= ops.INDEX_MAX_M:
            raise ValueError(f"search needs 1 <= m <= {ops.INDEX_MAX_M}, got m = {m}")
        c = mdl.cluster_centers_
        K, nprobe = int(c.shape[0]), int(nprobe)
        if not 1 <= nprobe <= K:
            raise ValueError(f"search needs 1 <= nprobe <= n_clusters ({K}), got nprobe = {nprobe}")
        if getattr(Q, "ndim", 2) != 2:
            raise ValueError(f"Q must be 2-D [n_queries, n_features], got shape {tuple(Q.shape)}")
        if refine is None and shortlist is not None:
            raise ValueError("search takes shortlist only with refine=X, the rows to re-rank on")
        if refine is not None:
            return self._search_refined(Q, m, nprobe, squared, refine, shortlist)
        if ix.codes.is_cuda:
            from .parallel import memplan

            plan = memplan.plan_pq_search(ix.n, int(c.shape[1]), K, ix.M, ix.dtype, nq=int(Q.shape[0]), m=m, nprobe=nprobe)
            plan.budget = memplan.hbm_budget(ix.codes.device) + sum(
                plan.persistent[k] for k in ("codes", "order", "offsets", "codebooks"))   # (held already)
            if not plan.fits:
                raise memplan.HBMCapacityError(f"search: {plan.summary()} does not fit")
        (keys,), was_numpy = mdl._row_blocks(Q, lambda Qt, pk: (ops.pq_search(ix, Qt, c, m, nprobe, pack=pk),))
        rows, d2 = ops.index_decode(keys, row_start=self.row_start)
        d = d2 if squared else d2.sqrt()
        return (rows.cpu().numpy(), d.cpu().numpy()) if was_numpy else (rows, d)

    def reconstruct(self, ids):
        """float32 ``[len, n_features]``: every row id's centre plus its codewords; NaN rows for ids in
        no list.  numpy in, numpy out."""
        was_numpy = not torch.is_tensor(ids)
        t = torch.as_tensor(np.asarray(ids)) if was_numpy else ids
        if t.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"reconstruct takes integer row ids, got {t.dtype}")
        ix = self._index
        out = ops.pq_reconstruct(ix, t.reshape(-1).to(device=ix.codes.device, dtype=torch.int64) - self.row_start,
                                 self._model.cluster_centers_)
        return out.cpu().numpy() if was_numpy else out

    def save(self, path):
        """Write the index to the directory ``path``: ``pq_index.safetensors`` (its tensors and the
        centres its rows were listed under) and ``pq_index.json`` (the format version and ``n``, ``K``,
        ``D``, ``M``, ``dtype``, ``row_start``)."""
        import json
        import os
        from pathlib import Path

        from safetensors.torch import save_file

        ix = self._index
        path = Path(path)
        path.mkdir(parents=True, exist_ok=True)
        blobs = {k: v.detach().to("cpu").contiguous() for k, v in ix.tensors().items()}
        blobs["centers"] = self._model.cluster_centers_.detach().to("cpu").contiguous()
        tmp = path / (self.TENSORS + ".tmp")
        save_file(blobs, str(tmp))
        os.replace(tmp, path / self.TENSORS)
        meta = {"format": self.FORMAT, "n": int(ix.n), "K": int(ix.K), "D": int(ix.D), "M": int(ix.M),
                "dtype": "bfloat16" if ix.dtype == torch.bfloat16 else "float32", "row_start": int(self.row_start)}
        tmpm = path / (self.META + ".tmp")
        tmpm.write_text(json.dumps(meta))
        os.replace(tmpm, path / self.META)
        return path

    @classmethod
    def saved_at(cls, path) -> bool:
        """Whether the directory ``path`` holds a saved PQ index."""
        from pathlib import Path

        return (Path(path) / cls.META).is_file() and (Path(path) / cls.TENSORS).is_file()

    @classmethod
    def load(cls, path, model, device=None) -> "PQIndex":
        """The index :meth:`save` wrote, for ``model`` (whose fitted centres must be the saved ones, bit
        for bit, and whose dtype the index's) on ``device`` (default: the model's).  It searches bit for
        bit as the saved one on the same kind of device."""
        import json
        from pathlib import Path

        from safetensors.torch import load_file

        model._check_fitted()
        comm = getattr(model, "comm", None) or get_comm()
        if _allreduce(comm) is not None:
            raise NotImplementedError("PQIndex.load is not available in a multi-rank job")
        path = Path(path)
        meta = json.loads((path / cls.META).read_text())
        if meta.get("format") != cls.FORMAT:
            raise ValueError(f"{path}: not a {cls.FORMAT} index (format {meta.get('format')!r})")
        c = model.cluster_centers_
        dev = torch.device(device) if device is not None else c.device
        ts = load_file(str(path / cls.TENSORS))
        saved_c = ts.pop("centers")
        dtype = torch.bfloat16 if meta["dtype"] == "bfloat16" else torch.float32
        if dtype != model.dtype:
            raise ValueError(f"the index holds {dtype} rows, the model's dtype is {model.dtype}")
        if saved_c.shape != c.shape or not torch.equal(saved_c, c.detach().to("cpu")):
            raise ValueError("the model's cluster_centers_ are not the centres the index was saved under")
        if dev.type != c.device.type:
            raise ValueError(f"the index would load to {dev}, the model's centres are on {c.device}")
        F = int(c.shape[1])
        D = int(pad_columns(torch.empty((0, F), dtype=dtype)).shape[1]) if dev.type == "cuda" else F
        ts = {k: v.to(dev) for k, v in ts.items()}
        index = ops.PQRowIndex(int(meta["n"]), int(meta["K"]), D, int(meta["M"]), dtype, ts["codes"], ts["order"],
                               ts["offsets"], ts["codebooks"])
        return cls(model, index, int(meta["row_start"]))


class _Params:
    """scikit-learn estimator protocol: ``get_params`` / ``set_params`` over the constructor's
    keyword arguments (so ``sklearn.base.clone``, pipelines and grid searches can rebuild an
    estimator), and a repr of the non-default ones."""

    @classmethod
    def _param_names(cls) -> list[str]:
        import inspect

        sig = inspect.signature(cls.__init__)
        return [n for n, p in sig.parameters.items() if n != "self" and p.kind == p.KEYWORD_ONLY
                or n == "n_clusters"]

    def get_params(self, deep: bool = True) -> dict:
        out = {}
        for n in self._param_names():
            if n == "random_state":
                out[n] = None          # (folded into seed by the constructor)
            else:
                out[n] = getattr(self, n, None)
        return out

    def set_params(self, **params):
        names = set(self._param_names())
        bad = [k for k in params if k not in names]
        if bad:
            raise ValueError(f"invalid parameter(s) {bad} for {type(self).__name__}")
        # validate / normalise through the constructor, then copy the parameters over
        ref = type(self)(**{**self.get_params(), **params})
        for n in names:
            if n != "random_state" and hasattr(ref, n):
                setattr(self, n, getattr(ref, n))
        return self

    def __repr__(self):
        import inspect

        sig = inspect.signature(type(self).__init__)
        cur = self.get_params()
        diff = [f"n_clusters={cur['n_clusters']}"]
        for n, p in sig.parameters.items():
            if n == "n_clusters":
                continue
            if n in cur and p.default is not inspect.Parameter.empty:
                v = cur[n]
                d = p.default
                if n == "dtype":
                    v, d = str(v).replace("torch.", ""), str(resolve_dtype(d)).replace("torch.", "")
                if isinstance(v, (int, float, str, bool, type(None))) and v != d:
                    diff.append(f"{n}={v!r}")
        return f"{type(self).__name__}({', '.join(diff)})"


class _Serving(_Params):
    """Inference surface shared by KMeans and MiniBatchKMeans (fitted ``cluster_centers_``)."""

    def _serving_pack(self, Xt):
        """The fitted centres packed for the assign kernel, built once and reused by every
        predict/score call until the centres change (serving: one kernel launch per batch)."""
        c = self.cluster_centers_
        if not Xt.is_cuda or not c.is_cuda:
            return None
        D = ops.pad_columns(Xt[:1]).shape[1]
        if ops.dpad_for(D, Xt.dtype) == 0:
            return None
        key = (c._version, Xt.dtype, D, Xt.device)
        cached = getattr(self, "_pack_cache", None)
        # (the cache holds the centres tensor itself: identity + version detect any change)
        if cached is None or cached[0] is not c or cached[1] != key:
            cached = (c, key, ops.pack_centers(c, D, Xt.dtype, Xt.device))
            self._pack_cache = cached
        return cached[2]

    def _inputs(self, X):
        """X on the model's device and dtype; unit rows for the cosine metric (on the GPU by
        the same kernel the fit normalised with)."""
        Xt, was_numpy = _to_tensor(X, self.cluster_centers_.device, self.dtype)
        if getattr(self, "metric", "euclidean") == "cosine":
            if Xt.is_cuda and native_dpad(Xt.shape[1], Xt.dtype):
                P = pad_columns(Xt)
                if torch.is_tensor(X) and P.data_ptr() == X.data_ptr():
                    P = P.clone()          # never normalise the caller's rows in place
                native_mod().row_normalize(P)
                Xt = P
            else:
                Xt = _unit_rows(Xt)
        return Xt, was_numpy

    def _host_blocks(self, X, block_rows: int | None = None):
        """``(start, Xt, pack)`` over the rows of X, ``Xt`` ready for the kernels
        (:meth:`_inputs`) and ``pack`` the serving pack.  Device rows and CPU models go through
        in one piece.  Host rows bound for a GPU model go through in blocks of ~256 MB (or
        ``block_rows``: a host-shard fit labels its rows in batch-sized blocks, the memory
        plan's), so a shard larger than HBM (a streamed fit's) is never copied to the device
        whole.  An empty X still gives one (empty) block."""
        dev = self.cluster_centers_.device
        n = X.shape[0]
        block = n
        if dev.type == "cuda" and not (torch.is_tensor(X) and X.device == dev):
            block = int(block_rows) if block_rows else max(1, (1 << 28) // max(1, X.shape[1] * 4))
        for i in range(0, max(n, 1), max(block, 1)):
            Xt, _ = self._inputs(X[i : i + block] if block < n else X)
            yield i, Xt, self._serving_pack(Xt)

    def _row_blocks(self, X, run, block_rows: int | None = None):
        """``run(Xt, pack)`` -- a tuple of per-row tensors (or None) -- over every row of X
        (:meth:`_host_blocks`): ``(outputs, was_numpy)``."""
        n = X.shape[0]
        outs = None
        for i, Xt, pk in self._host_blocks(X, block_rows):
            part = run(Xt, pk)
            if Xt.shape[0] == n:
                outs = part
                break
            if outs is None:
                outs = [None if p is None else torch.empty((n, *p.shape[1:]), dtype=p.dtype, device=p.device)
                        for p in part]
            for o, p in zip(outs, part):
                if o is not None:
                    o[i : i + Xt.shape[0]] = p
        return tuple(outs), not torch.is_tensor(X)

    def _assign_rows(self, X, with_dist: bool, block_rows: int | None = None):
        """(labels, squared distances or None) of every row of X under the fitted centres
        (host rows in blocks, :meth:`_row_blocks`)."""
        (lab, mind), was_numpy = self._row_blocks(
            X, lambda Xt, pk: ops.assign(Xt, self.cluster_centers_, with_dist=with_dist, pack=pk), block_rows)
        return lab, mind, was_numpy

    def predict_topk(self, X, m: int, *, squared: bool = False, block_rows: int | None = None):
        """The ``m`` nearest centres of every row with their distances: ``(labels [n, m]
        int32, distances [n, m] float32)``, nearest first and equal distances by centre index.
        Distances are Euclidean as in :meth:`transform` (``squared``: the kernel's squared
        values; for the cosine metric between unit rows and unit centres).  On the GPU the
        fused top-m kernel on the serving pack (csrc/topk.hip) -- the ``[n, K]`` distance
        matrix is never written.  A row with a NaN or infinite coordinate gets NaN or inf
        distances, never 0, and a centre with one gets them from every row: such a centre
        sorts behind every finite distance (inf, then NaN).  The folds that read this
        (:meth:`cluster_report`, :meth:`cluster_exemplars`, :meth:`cluster_quantiles`,
        :meth:`build_index`) leave such rows out.  numpy in, numpy out; host rows bound for a
        GPU model go through in blocks (``block_rows``) as in :meth:`predict`."""
        self._check_fitted()
        m = int(m)
        K = int(self.cluster_centers_.shape[0])
        if not 1 <= m <= K:
            raise ValueError(f"predict_topk needs 1 <= m <= n_clusters ({K}), got m = {m}")
        (idx, d2), was_numpy = self._row_blocks(
            X, lambda Xt, pk: ops.topk(Xt, self.cluster_centers_, m, pack=pk), block_rows)
        d = d2 if squared else d2.sqrt()
        return (idx.cpu().numpy(), d.cpu().numpy()) if was_numpy else (idx, d)

    def cluster_report(self, X, *, block_rows: int | None = None) -> ClusterReport:
        """Per-cluster quality of ``X`` under the fitted centres, a :class:`ClusterReport`:
        every cluster's size, inertia, mean and rms distance, radius and simplified
        silhouette, and the totals (inertia, silhouette, Davies-Bouldin index, balance).

        One fused pass: the top-2 kernel (:meth:`predict_topk`'s, on the serving pack) gives
        each row's nearest and second-nearest centre, and csrc/quality.hip folds them into an
        integer table per cluster -- no ``[n, K]`` matrix, no floating-point add on the
        reduction path, so the report is bitwise the same from run to run, for any
        ``block_rows`` (rows per top-2 pass; host rows bound for a GPU model are also copied
        in blocks of that size) and, in a multi-rank job where ``X`` is the rank's shard, on
        any world size (the table is all-reduced; every rank returns the same report).

        A row's cluster is :meth:`predict_topk`'s first column: the exact nearest centre, the
        lower index on ties.  For bfloat16 that can differ from :meth:`predict` on near-ties,
        which ranks by packed keys.  Cosine models report on unit rows.  numpy in, numpy out."""
        self._check_fitted()
        c = self.cluster_centers_

        def fold(table):
            for _, Xt, pk in self._host_blocks(X, block_rows):
                ops.quality_rows(table, Xt, c, pack=pk, block_rows=block_rows)

        rep = _report_table(c, getattr(self, "comm", None) or get_comm(), self.dtype, fold)
        return rep if torch.is_tensor(X) else rep.numpy()

    def cluster_exemplars(self, X, m: int, *, farthest: bool = False, squared: bool = False,
                          block_rows: int | None = None):
        """For every cluster the ``m`` rows of ``X`` assigned to it that lie nearest its centre
        (``farthest``: the ``m`` farthest): ``(rows [K, m] int64, distances [K, m] float32)``.
        Nearest lists are in ascending, farthest lists in descending order of distance, equal
        distances by the lower row index; a cluster with fewer than ``m`` rows is padded with row
        -1 and distance NaN.  ``m`` counts rows, not centres: 1 <= m <= 64, and it may exceed
        ``n_clusters``.  Distances are Euclidean as in :meth:`transform` / :meth:`predict_topk`
        (``squared``: the kernel's squared values; cosine models work on unit rows).

        One pass over ``X`` and no sort of its rows: the top-1 kernel (:meth:`predict_topk`'s, on
        the serving pack) gives each row's centre and squared distance, and csrc/exemplars.hip
        min-inserts (distance bits, row) keys into an integer ``[K, m]`` table with 64-bit atomic
        min.  The result is bitwise the same from run to run and for any ``block_rows`` (rows per
        top-1 pass; host rows bound for a GPU model are also copied in blocks of that size).  In
        a multi-rank job ``X`` is the rank's shard, the row index is the global one (shard start
        + local index) and every rank returns the same lists: those of a one-rank call on the
        concatenated shards.  One call takes fewer than 2^32 rows.

        A row's cluster and distance are :meth:`predict_topk`'s first column: the exact nearest
        centre, the lower index on ties, as in :meth:`cluster_report`.  For bfloat16 that can
        differ from :meth:`predict` on near-ties, which ranks by packed keys.  Rows whose
        distance is NaN or infinite are in no list.  numpy in, numpy out."""
        self._check_fitted()
        c = self.cluster_centers_

        def fold(table):
            for start, Xt, pk in self._host_blocks(X, block_rows):
                ops.exemplar_rows(table, Xt, c, row0=start, farthest=farthest, pack=pk, block_rows=block_rows)

        rows, d = _exemplar_lists(c.shape[0], m, c.device, getattr(self, "comm", None) or get_comm(),
                                  X.shape[0], farthest, squared, fold)
        return (rows, d) if torch.is_tensor(X) else (rows.cpu().numpy(), d.cpu().numpy())

    def cluster_quantiles(self, X, q=(0.5, 0.9, 0.99), *, squared: bool = False, block_rows: int | None = None):
        """Exact per-cluster distance quantiles of ``X`` under the fitted centres: ``(values
        [K, Q] float32, counts [K] int64)``.  ``values[k, j]`` is the distance below or at which a
        share ``q[j]`` of the rows assigned to cluster ``k`` lie: the element at sorted position
        ``clamp(ceil(q * n_k) - 1, 0, n_k - 1)`` of the cluster's distances (the "inverted CDF"
        quantile: a real row's distance, never interpolated; ``q = 0`` the nearest row, ``q = 1``
        the farthest), ``counts[k] = n_k`` the rows counted; a cluster without rows gives NaN.
        ``q``: a number or up to 8 of them, each in [0, 1].  Distances are Euclidean as in
        :meth:`transform` / :meth:`predict_topk` (``squared``: the kernel's squared values; cosine
        models work on unit rows).

        No sort: the top-1 kernel (:meth:`predict_topk`'s, on the serving pack) runs once and its
        label and squared distance are kept (8 B per row on the device); csrc/quantiles.hip then
        selects by radix over the distance bits, four passes of per-cluster 256-bin histograms
        filled with integer atomics.  The result is bitwise the same from run to run and for any
        ``block_rows`` (rows per top-1 pass; host rows bound for a GPU model are also copied in
        blocks of that size).  In a multi-rank job ``X`` is the rank's shard, every pass's
        histogram is all-reduced and every rank returns the one-rank result on the concatenated
        shards.

        A row's cluster and distance are :meth:`predict_topk`'s first column: the exact nearest
        centre, the lower index on ties, as in :meth:`cluster_report`.  Rows whose distance is NaN
        or infinite are not counted.  numpy in, numpy out."""
        self._check_fitted()
        c = self.cluster_centers_
        qs = ops.quantile_levels(q)
        chunks = []
        for _, Xt, pk in self._host_blocks(X, block_rows):
            chunks.extend(ops.quantile_top1(Xt, c, pack=pk, block_rows=block_rows))
        reduce = _allreduce(getattr(self, "comm", None) or get_comm())
        v, counts = ops.quantile_passes(chunks, c.shape[0], qs, c.device, reduce=reduce)
        v = v if squared else v.sqrt()
        return (v, counts) if torch.is_tensor(X) else (v.cpu().numpy(), counts.cpu().numpy())

    def build_index(self, X, *, block_rows: int | None = None) -> ClusterIndex:
        """Index the rows of ``X`` by their nearest fitted centre, for :meth:`ClusterIndex.search`:
        the fitted model as the coarse quantiser of an inverted-file (IVF-Flat) index.

        A row's list is :meth:`predict_topk`'s first column (the exact nearest centre, the lower
        index on ties, as in :meth:`cluster_report`); rows whose distance to it is NaN or infinite are
        in no list; a list holds its rows in ascending row index.  Cosine models index unit rows.
        On the GPU the rows are grouped by a native stable partition (csrc/ivf.hip: count, scan,
        scatter; no atomic decides a position) and packed list after list in the layout the MFMA
        kernels read centres in, each row read once in its own dtype.  The index is bitwise the
        same from run to run and for any ``block_rows`` (rows per top-1 pass; host rows bound for
        a GPU model are also copied in blocks of that size, twice: once for the lists, once for
        the pack).  In a multi-rank job ``X`` is the rank's shard and row ids are global.  One index
        takes fewer than 2^32 rows; on a GPU its memory plan (``memplan.plan_index``) is checked
        against the HBM budget up front."""
        self._check_fitted()
        c = self.cluster_centers_
        n = int(X.shape[0])
        if n >= 1 << 32:
            raise ValueError(f"build_index takes fewer than 2^32 rows, got {n}")
        if c.is_cuda:
            from .parallel import memplan

            plan = memplan.plan_index(n, int(X.shape[1]), int(c.shape[0]), self.dtype, block_rows=block_rows)
            plan.budget = memplan.hbm_budget(c.device)
            if not plan.fits:
                raise memplan.HBMCapacityError(f"build_index: {plan.summary()} does not fit")
        comm = getattr(self, "comm", None) or get_comm()
        start = _shard_info(n, comm, c.device)[1] if _allreduce(comm) is not None else 0
        index = ops.index_build(None, c, block_rows=block_rows, n=n,
                                blocks=lambda: self._host_blocks(X, block_rows))
        return ClusterIndex(self, index, start, comm)

    def load_index(self, path) -> ClusterIndex:
        """The index :meth:`ClusterIndex.save` wrote to ``path``, on this model's device
        (:meth:`ClusterIndex.load`): the fitted centres must be the ones it was saved under."""
        return ClusterIndex.load(path, self)

    def build_pq_index(self, X, n_subvectors: int = 16, *, train_rows: int = 65536, pq_max_iter: int = 25,
                       seed: int | None = None, codebooks=None, block_rows: int | None = None) -> PQIndex:
        """Index the rows of ``X`` by their nearest fitted centre and keep each as ``n_subvectors``
        one-byte codes of its residual against that centre (product quantisation), for
        :meth:`PQIndex.search`: ``n_subvectors`` bytes a row where :meth:`build_index` keeps the row.

        ``n_subvectors`` in {8, 16, 32, 64} must divide the features.  The lists are
        :meth:`build_index`'s (cosine models index unit rows; a row whose distance to its centre is NaN
        or infinite takes an id and is in no list).  The 256 codewords of every sub-space are fitted by
        this library's own :class:`KMeans` (``pq_max_iter`` iterations) on the residuals of
        ``min(train_rows, n_indexed)`` listed rows drawn under ``seed`` (default: the model's), or
        given as ``codebooks`` float32 ``[n_subvectors, 256, dsub]``; a code is the exact nearest
        codeword (the top-1 kernel).  The index is bitwise the same from run to run and for any
        ``block_rows``.  numpy or torch, host or device rows (host rows bound for a GPU model cross in
        blocks).  One-rank jobs only; on a GPU the memory plan (``memplan.plan_pq_index``) is checked
        against the HBM budget up front."""
        self._check_fitted()
        comm = getattr(self, "comm", None) or get_comm()
        if _allreduce(comm) is not None:
            raise NotImplementedError("build_pq_index is not available in a multi-rank job")
        c = self.cluster_centers_
        n, M = int(X.shape[0]), int(n_subvectors)
        if getattr(X, "ndim", 0) != 2 or int(X.shape[1]) != int(c.shape[1]):
            raise ValueError(f"build_pq_index takes rows [n, {int(c.shape[1])}], got shape {tuple(getattr(X, 'shape', ()))}")
        ops.pq_check(int(c.shape[1]), M)
        if n >= 1 << 32:
            raise ValueError(f"build_pq_index takes fewer than 2^32 rows, got {n}")
        if c.is_cuda:
            from .parallel import memplan

            plan = memplan.plan_pq_index(n, int(c.shape[1]), int(c.shape[0]), M, self.dtype, block_rows=block_rows,
                                         train_rows=train_rows)
            plan.budget = memplan.hbm_budget(c.device)
            if not plan.fits:
                raise memplan.HBMCapacityError(f"build_pq_index: {plan.summary()} does not fit")
        if codebooks is not None:
            codebooks = torch.as_tensor(np.asarray(codebooks) if not torch.is_tensor(codebooks) else codebooks,
                                        dtype=torch.float32)
        seed = int(getattr(self, "seed", 0) or 0) if seed is None else int(seed)
        index = ops.pq_build(None, c, M, codebooks=codebooks, train_rows=train_rows, max_iter=pq_max_iter, seed=seed,
                             block_rows=block_rows, n=n, blocks=lambda: self._host_blocks(X, block_rows))
        return PQIndex(self, index, 0)

    def load_pq_index(self, path) -> PQIndex:
        """The index :meth:`PQIndex.save` wrote to ``path``, on this model's device
        (:meth:`PQIndex.load`): the fitted centres must be the ones it was saved under."""
        return PQIndex.load(path, self)

    def transform(self, X):
        """Euclidean distances to every centre, ``[n, K]`` (float32; for the cosine
        metric, between unit rows and unit centres: sqrt(2 - 2 cos)).  On the GPU: the MFMA
        transform kernel on the serving pack (csrc/transform.hip).  A row or a centre with a NaN
        or infinite coordinate gives NaN or inf in its row or column, never 0, and changes no
        other entry."""
        self._check_fitted()
        Xt, was_numpy = self._inputs(X)
        d = ops.transform(Xt, self.cluster_centers_, pack=self._serving_pack(Xt))
        return d.cpu().numpy() if was_numpy else d

    def fit_transform(self, X, *args, **kw):
        """``fit(X)`` then the distances of ``X`` to the fitted centres."""
        return self.fit(X, *args, **kw).transform(X)

    def _check_fitted(self):
        if not hasattr(self, "cluster_centers_"):
            raise RuntimeError(f"{type(self).__name__} instance is not fitted yet; call fit() first")


class KMeans(_Serving):
    """Lloyd k-means on MI355X (full batch, data-parallel over ranks)."""

    def __init__(self, n_clusters: int = 8, *, init="k-means++", n_init: int = 1, max_iter: int = 300,
                 tol: float = 1e-4, dtype="float32", device=None, seed: int | None = 0,
                 random_state: int | None = None, comm: Comm | None = None, frozen=None,
                 empty_cluster: str = "keep", check_every: int = 1, n_local_trials=None,
                 verbose: int = 0, mode: str = "learn", run_id: str | None = None,
                 checkpoint_every: int = 0, checkpoint_dir: str | None = None, metrics_path: str | None = None,
                 graph: bool = False, incremental: bool = True, chunk_rows: int | None = None,
                 init_size: int | None = None, metric: str = "euclidean", algorithm: str = "auto",
                 init_sampling: str = "exact"):
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.dtype = resolve_dtype(dtype)
        self.device = device
        self.seed = int(random_state if random_state is not None else (seed or 0))
        self.comm = comm
        self.frozen = frozen
        self.empty_cluster = empty_cluster
        self.check_every = int(check_every)
        self.n_local_trials = n_local_trials
        self.verbose = verbose
        self.mode = mode
        self.run_id = run_id
        self.checkpoint_every = int(checkpoint_every)
        self.checkpoint_dir = checkpoint_dir
        self.metrics_path = metrics_path
        self.graph = bool(graph)
        self.incremental = bool(incremental)
        # out-of-core fits (models/streaming.py): X stays in host memory and streams through
        # the GPU in chunks of `chunk_rows`; the init (and tol scale) use `init_size` rows
        self.chunk_rows = int(chunk_rows) if chunk_rows else None
        if metric not in ("euclidean", "cosine"):
            raise ValueError(f"metric must be 'euclidean' or 'cosine', got {metric!r}")
        # cosine = spherical k-means: unit rows, centres re-normalised after every M-step
        self.metric = metric
        # 'hamerly' (sklearn's 'elkan' maps here too): the GPU E-step keeps per-row distance
        # bounds and re-assigns only the rows they cannot vouch for (models/lloyd.py) -- the
        # full E-step's labels bit for bit (tests/test_gpu_bounded.py), far fewer MFMA passes
        # once few rows move.  'auto' (default): 'hamerly' wherever the memory plan holds the
        # bounds resident (~21 B/row) and the options are the bounded path's, else 'lloyd';
        # the choice is agreed by every rank and reported as ``algorithm_``.
        algo = {"elkan": "hamerly", "full": "lloyd"}.get(algorithm, algorithm)
        if algo not in ("auto", "lloyd", "hamerly"):
            raise ValueError(f"algorithm must be 'auto', 'lloyd' or 'hamerly' ('elkan'), got {algorithm!r}")
        self.algorithm = algo
        self.algorithm_ = None
        # multi-rank k-means++: 'exact' (world-size invariant, two collectives per centre) or
        # 'two-stage' (one all-gather per centre; models/init.py)
        if init_sampling not in ("exact", "two-stage"):
            raise ValueError(f"init_sampling must be 'exact' or 'two-stage', got {init_sampling!r}")
        self.init_sampling = init_sampling
        self.init_size = init_size
        self.history_: list[dict] = []

    # ---------------------------------------------------------------- config
    @classmethod
    def from_config(cls, cfg: KMeansConfig, **kw):
        return cls(n_clusters=cfg.n_clusters, init=cfg.init, n_init=cfg.n_init, max_iter=cfg.max_iter,
                   tol=cfg.tol, dtype=cfg.dtype, device=cfg.device, seed=cfg.seed,
                   empty_cluster=cfg.empty_cluster, check_every=cfg.check_every,
                   n_local_trials=cfg.n_local_trials, verbose=cfg.verbose, mode=cfg.mode,
                   run_id=cfg.run_id, checkpoint_every=cfg.checkpoint_every,
                   checkpoint_dir=cfg.checkpoint_dir, metrics_path=cfg.metrics_path, graph=cfg.graph,
                   incremental=cfg.incremental, chunk_rows=cfg.chunk_rows, metric=cfg.metric,
                   algorithm=cfg.algorithm, init_sampling=cfg.init_sampling, **kw)

    def get_config(self) -> KMeansConfig:
        return KMeansConfig(n_clusters=self.n_clusters, init=self.init if isinstance(self.init, str) else "array",
                            n_init=self.n_init, max_iter=self.max_iter, tol=self.tol,
                            dtype="bfloat16" if self.dtype == torch.bfloat16 else "float32",
                            device=str(self.device) if self.device else None, seed=self.seed,
                            empty_cluster=self.empty_cluster, check_every=self.check_every,
                            n_local_trials=self.n_local_trials, mode=self.mode, run_id=self.run_id,
                            verbose=self.verbose, checkpoint_every=self.checkpoint_every,
                            checkpoint_dir=self.checkpoint_dir, metrics_path=self.metrics_path,
                            graph=self.graph, incremental=self.incremental, chunk_rows=self.chunk_rows,
                            metric=self.metric, algorithm=self.algorithm, init_sampling=self.init_sampling)

    # ------------------------------------------------------------------- fit
    AUTO_MIN_ROWS = 1 << 16      # per rank: below it the full E-step's pass costs less than the bounds
    AUTO_MIN_CLUSTERS = 32

    def _auto_bounded_ok(self, n_local: int, weighted: bool) -> bool:
        """This rank's vote for the bounded E-step under algorithm='auto': the option set the
        bounded path covers bit for bit (plain Euclidean, unweighted, 'keep' empty clusters, an
        in-HBM shard) and a problem big enough for the bounds to pay."""
        return (self.metric == "euclidean" and not weighted and self.empty_cluster == "keep"
                and self.chunk_rows is None and n_local >= self.AUTO_MIN_ROWS
                and self.n_clusters >= self.AUTO_MIN_CLUSTERS)

    def _memory_plan(self, X, comm, device, D, weighted):
        """Resident or streamed (parallel/memplan.py), agreed by every rank: a rank whose
        shard does not fit makes all of them stream (the init sample and its collectives
        must match).  ``chunk_rows`` forces streaming with that chunk."""
        from .parallel import memplan

        n_local = int(X.shape[0])
        self.algorithm_ = "hamerly" if self.algorithm == "hamerly" else "lloyd"
        es_src = X.element_size() if torch.is_tensor(X) else np.asarray(X).itemsize
        x_dev = torch.is_tensor(X) and X.is_cuda
        kw = dict(weighted=weighted, init=self.init, n_local_trials=self.n_local_trials,
                  empty_policy=self.empty_cluster)
        budget = memplan.hbm_budget(device)
        if self.chunk_rows is not None and not x_dev:
            plan = memplan.plan_streaming(n_local, D, self.n_clusters, self.dtype, chunk_rows=self.chunk_rows,
                                          init_rows=self.init_size, src_itemsize=es_src, **kw)
            plan.budget = budget
            # every rank learns whether any forced chunk does not fit (one collective, as below)
            flags = torch.tensor([0.0 if plan.fits else 1.0], dtype=torch.float64, device=comm.device)
            comm.allreduce_max_(flags)
            if flags[0].item() > 0:
                raise memplan.HBMCapacityError(
                    f"KMeans.fit: chunk_rows={self.chunk_rows} does not fit "
                    + (plan.summary() if not plan.fits else "another rank's HBM budget")
                    + "; use a smaller chunk_rows or more ranks")
        else:
            fit_kw = dict(budget=budget, x_on_device=x_dev, incremental=self.incremental, init_rows=self.init_size,
                          src_itemsize=es_src, copy_x=not self._x_ready(X, device), **kw)
            auto_b = self.algorithm == "auto" and self._auto_bounded_ok(n_local, weighted)
            plan = None
            if auto_b:
                try:   # the bounds must fit beside a resident shard, else the plain plan decides
                    plan = memplan.plan_fit(n_local, D, self.n_clusters, self.dtype, bounded=True, **fit_kw)
                    auto_b = plan.mode == "resident"
                except memplan.HBMCapacityError:
                    auto_b = False
                if not auto_b:
                    plan = None
            try:
                if plan is None:
                    plan = memplan.plan_fit(n_local, D, self.n_clusters, self.dtype,
                                            bounded=self.algorithm == "hamerly", **fit_kw)
                err = 0.0
            except memplan.HBMCapacityError as e:
                plan, err = e, 1.0
            no_b = 0.0 if (auto_b or self.algorithm == "hamerly") else 1.0
            flags = torch.tensor([err, 1.0 if (err == 0.0 and plan.mode == "streaming") else 0.0, no_b],
                                 dtype=torch.float64, device=comm.device)
            comm.allreduce_max_(flags)
            if self.algorithm == "auto" and flags[2].item() == 0.0:
                self.algorithm_ = "hamerly"     # every rank voted for the bounds (and holds them)
            if flags[0].item() > 0:
                raise plan if isinstance(plan, memplan.HBMCapacityError) else memplan.HBMCapacityError(
                    "KMeans.fit: another rank's shard does not fit its HBM budget")
            if flags[1].item() > 0:
                # some rank streams: all must (the init sample and its collectives must match);
                # a second agreement, so a rank that cannot follow fails every rank together
                msg = None
                if plan.mode != "streaming":
                    if x_dev:
                        msg = ("KMeans.fit: other ranks stream their shards; pass this rank's rows as a host "
                               "tensor too")
                    else:
                        try:
                            plan = self._stream_plan(n_local, D, es_src, budget, kw)
                        except memplan.HBMCapacityError as e:
                            msg = str(e)
                f2 = torch.tensor([1.0 if msg else 0.0], dtype=torch.float64, device=comm.device)
                comm.allreduce_max_(f2)
                if f2[0].item() > 0:
                    raise memplan.HBMCapacityError(msg or "KMeans.fit: another rank cannot stream its shard")
        if self.verbose and comm.rank == 0:
            print(f"[mikmeans] memory plan: {plan.summary()}", flush=True)
        return plan

    def _stream_plan(self, n_local, D, es_src, budget, kw):
        from .parallel import memplan

        R = memplan.ROW_ALIGN
        while R * 2 <= (1 << 24) and R < n_local:
            R *= 2
        while True:
            pl = memplan.plan_streaming(n_local, D, self.n_clusters, self.dtype, chunk_rows=R,
                                        init_rows=self.init_size, src_itemsize=es_src, **kw)
            pl.budget = budget
            if pl.fits:
                return pl
            if R <= memplan.ROW_ALIGN:
                # (another rank chose streaming and this one cannot stream within its budget)
                raise memplan.HBMCapacityError(f"KMeans.fit: {pl.summary()} does not fit even in "
                                               f"{memplan.ROW_ALIGN}-row chunks")
            R //= 2

    def _x_ready(self, X, device) -> bool:
        """X is already the device tensor the resident engine computes on (no copy made)."""
        if not (torch.is_tensor(X) and X.device == device and X.dtype == self.dtype) or self.metric == "cosine":
            return False
        return pad_columns(X[:0]).data_ptr() == X[:0].data_ptr() if X.shape[0] else True

    def fit(self, X, y=None, sample_weight=None, *, resume_from=None):
        """Lloyd fit.  On a GPU the memory plan (``memory_plan_``) decides whether the shard
        is copied into HBM or streamed from host memory chunk by chunk; both give the same
        model from the same start (init 'random', an array, or a resumed checkpoint;
        k-means++ seeds a streamed fit from an ``init_size``-row sample)."""
        comm = self.comm or get_comm()
        device = _default_device(self.device, X) if self.device is not None or comm.world == 1 else comm.device
        if not torch.is_tensor(X):
            X = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32)
                                                      if np.asarray(X).dtype not in (np.float32, np.float64)
                                                      else np.asarray(X)))
            self._numpy_io = True
        else:
            self._numpy_io = False
        if X.dim() != 2:
            raise ValueError(f"X must be 2-D [n_samples, n_features], got shape {tuple(X.shape)}")
        D = int(X.shape[1])
        w = None
        if sample_weight is not None:
            w = torch.as_tensor(np.asarray(sample_weight) if not torch.is_tensor(sample_weight)
                                else sample_weight, dtype=torch.float32)
        gpu = device.type == "cuda" and native_dpad(D, self.dtype) != 0
        self.memory_plan_ = None
        self.algorithm_ = "hamerly" if self.algorithm == "hamerly" else "lloyd"
        streaming = False
        if gpu:
            plan = self._memory_plan(X, comm, device, D, w is not None)
            self.memory_plan_ = plan.as_dict()
            streaming = plan.mode == "streaming"
        n_global, start = _shard_info(X.shape[0], comm, comm.device)
        if n_global < self.n_clusters:
            raise ValueError(f"n_samples={n_global} should be >= n_clusters={self.n_clusters}")
        spherical = self.metric == "cosine"
        if streaming:
            from .models.streaming import StreamingLloydEngine

            Xh = X if X.device.type == "cpu" else X.cpu()
            sengine = StreamingLloydEngine(Xh, self.n_clusters, chunk_rows=plan.chunk_rows, comm=comm,
                                           device=device, frozen=self.frozen, n_features=D, dtype=self.dtype,
                                           sample_weight=w, empty_policy=self.empty_cluster, spherical=spherical)
            tol_abs = tol_to_abs(self.tol, None, comm, n_global, D, stats=sengine.stats)
            Xt = None
        else:
            Xt = _device_rows(X, device, self.dtype, gpu)
            if spherical:
                if gpu:
                    if Xt is X:
                        Xt = Xt.clone()
                    from .ops import native as _nat

                    _nat.require().row_normalize(Xt)
                else:
                    Xt = _unit_rows(Xt)
            if w is not None:
                w = w.to(device)
        best = None
        t0 = time.perf_counter()
        start_iter = 0
        for trial in range(max(1, self.n_init)):
            if streaming:
                eng = sengine
                eng.reset_labels()
            else:
                eng = LloydEngine(Xt, self.n_clusters, comm=comm, sample_weight=w, frozen=self.frozen,
                                  empty_policy=self.empty_cluster, n_features=D, incremental=self.incremental,
                                  spherical=spherical, bounded=self.algorithm_ == "hamerly")
                if trial == 0:
                    stats = eng.stats if eng.gpu else None
                    tol_abs = tol_to_abs(self.tol, Xt, comm, n_global, D, stats=stats)
            if resume_from is not None and trial == 0:
                from .utils.checkpoint import load_checkpoint

                ck = load_checkpoint(resume_from, comm=comm)
                centers = ck["centers"].to(device)
                start_iter = int(ck["iteration"])
            else:
                centers = self._init_centers(eng if streaming else Xt, streaming, D, n_global, start, comm,
                                             trial)
            eng.set_centers(centers[:, :D])
            eng.iteration = start_iter
            hist = []
            mlog = mmetrics.MetricsLogger(self.metrics_path, rank=comm.rank, world=comm.world,
                                          n_points=n_global, run_id=self.run_id) if self.metrics_path else None

            def cb(st, _eng=eng, _hist=hist, _mlog=mlog):
                rec = st.as_dict()
                counts = _eng.counts.tolist() if (self.verbose > 1 or _mlog is not None) else None
                rec["counts"] = counts if self.verbose > 1 else None
                if getattr(_eng, "bounded", False):
                    rec["reassigned"] = _eng.reassigned     # rows the bounded E-step re-assigned
                _hist.append(rec)
                if _mlog is not None:
                    _mlog.log(st, counts)
                faults.maybe_fail(comm.rank, st.iteration)
                if self.verbose and comm.rank == 0:
                    what = (f"reassigned {rec['reassigned']}" if "reassigned" in rec
                            else f"inertia {st.inertia:.6g}")
                    print(f"[mikmeans] iter {st.iteration} {what} shift {st.shift:.3g} changed {st.n_changed}",
                          flush=True)
                if self.checkpoint_every and self.checkpoint_dir and st.iteration % self.checkpoint_every == 0:
                    from .utils.checkpoint import save_checkpoint

                    # Lloyd draws random numbers only while seeding (Philox / seeded NumPy keyed
                    # by config.seed and the trial); a resumed run continues from the centres
                    save_checkpoint(self.checkpoint_dir, _eng.centers, st.iteration, self.get_config(),
                                    history=_hist, comm=comm,
                                    extra={"rng": {"scheme": "seeding only, keyed by (seed, trial)",
                                                   "seed": self.seed, "trial": trial}})

            if self.graph:
                eng.capture()
            remaining = max(0, self.max_iter - start_iter)
            n_iter, converged, _ = eng.run(remaining, tol_abs, check_every=self.check_every, callback=cb)
            if mlog is not None:
                mlog.close()
            labels, mind = eng.assign(True)
            inert = torch.zeros(1, dtype=torch.float64, device=eng.device)
            if eng.n:
                if eng.weights is not None and eng.gpu:
                    C_ = native_mod()
                    C_.wdot(mind, eng.weights, inert,
                            torch.empty(C_.WDOT_SCRATCH, dtype=torch.float64, device=mind.device))
                elif eng.weights is not None:
                    inert += (mind.double() * eng.weights.double()).sum().to(inert.device)
                else:
                    inert += mind.sum(dtype=torch.float64).to(inert.device)
            del mind
            inert = inert.to(comm.device)
            comm.allreduce_(inert)
            inertia = float(inert.item())
            if best is None or inertia < best[0]:
                best = (inertia, eng, labels, n_iter, converged, hist)
                if streaming:   # the engine is reused by the next trial: keep this one's centres
                    best = best + (eng.centers.clone(),)
        inertia, eng, labels, n_iter, converged, hist = best[:6]
        self._engine = eng
        self.cluster_centers_ = best[6] if streaming else eng.centers.clone()
        self.labels_ = labels
        self.inertia_ = inertia
        self.n_iter_ = n_iter
        self.converged_ = converged
        self.history_ = hist
        self.n_features_in_ = D
        self.fit_time_s_ = time.perf_counter() - t0
        cnt = torch.bincount(labels, minlength=self.n_clusters).to(torch.float64).to(comm.device)
        comm.allreduce_(cnt)
        self.counts_ = cnt.cpu()
        return self

    def _init_centers(self, src, streaming: bool, D: int, n_global: int, start: int, comm, trial: int):
        """Initial centres.  Streamed shards: 'random' draws its rows from the whole shard
        (fetched from host memory, so the resident fit's rows), k-means++ runs on a
        device-resident ``init_size``-row sample of every rank's rows."""
        seed = self.seed + trial
        if not streaming:
            return resolve_init(self.init, src, D, self.n_clusters, n_global, start, comm, seed,
                                self.n_local_trials, sampling=self.init_sampling)
        name = self.init.lower().replace("_", "-") if isinstance(self.init, str) else None
        if name == "random":
            from .models.init import init_random

            return init_random(None, D, self.n_clusters, n_global, start, comm, seed, fetch=src.fetch_rows,
                               n_local=src.n)
        if name is None:
            return resolve_init(self.init, src.fetch_rows([]), D, self.n_clusters, n_global, start, comm,
                                seed, self.n_local_trials)
        m = self.init_size or max(20 * self.n_clusters, 1 << 16)
        Xs = src.sample_rows(m, self.seed)
        s_global, s_start = _shard_info(Xs.shape[0], comm, comm.device)
        return resolve_init(self.init, Xs, D, self.n_clusters, s_global, s_start, comm, seed,
                            self.n_local_trials, sampling=self.init_sampling)

    def fit_predict(self, X, y=None, sample_weight=None):
        return self.fit(X, sample_weight=sample_weight)._out(self.labels_)

    # --------------------------------------------------------------- predict
    def reset(self):
        """Forget the fit (the reference's hard reset, app.mjs:225-237); keeps the config."""
        for k in ("cluster_centers_", "labels_", "inertia_", "n_iter_", "converged_", "counts_",
                  "n_features_in_", "fit_time_s_", "_engine"):
            self.__dict__.pop(k, None)
        self.history_ = []
        return self

    def _out(self, t):
        if getattr(self, "_numpy_io", False):
            return t.cpu().numpy()
        return t

    def predict(self, X, *, unassign_nonfinite: bool = False):
        """Nearest-centre labels.  ``unassign_nonfinite`` gives rows with NaN/inf
        coordinates the label -1 ("unassigned", the reference's unassigned list,
        app.mjs:421-433); the M-step ignores such labels.  So does a row whose float32
        squared norm overflows (a coordinate of 1e20): its distance to every centre is inf,
        :meth:`predict_topk` and the folds treat it as non-finite, and no centre is its
        nearest.  Without the flag the labels of such rows are unspecified; the other rows
        keep theirs either way."""
        self._check_fitted()
        labels, _, was_numpy = self._assign_rows(X, False)
        if unassign_nonfinite:
            Xt = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X)
            # (a NaN or infinite coordinate makes the sum of squares NaN or inf as well)
            bad = (~torch.isfinite(Xt.to(torch.float32).square().sum(dim=1))).to(labels.device)
            labels = labels.masked_fill(bad, -1)
        return labels.cpu().numpy() if was_numpy else labels

    def score(self, X, sample_weight=None):
        """Negative inertia of ``X`` under the fitted centres."""
        self._check_fitted()
        _, mind, _ = self._assign_rows(X, True)
        if sample_weight is not None:
            mind = mind * torch.as_tensor(np.asarray(sample_weight), dtype=torch.float32, device=mind.device)
        return -float(mind.sum(dtype=torch.float64))

    # --------------------------------------------------------------- metrics
    def metrics(self) -> dict:
        """Dashboard metrics of the fit (reference snapshotMetrics parity, app.mjs:481-496)."""
        self._check_fitted()
        counts = [int(c) for c in self.counts_.tolist()]
        return {
            "k": self.n_clusters,
            "counts": counts,
            "balance": mmetrics.balance(counts),
            "inertia": self.inertia_,
            "n_iter": self.n_iter_,
        }

    # ------------------------------------------------------------- persist
    def save(self, path):
        from .utils.checkpoint import save_checkpoint

        self._check_fitted()
        return save_checkpoint(path, self.cluster_centers_, self.n_iter_, self.get_config(),
                               history=self.history_, comm=self.comm or get_comm())

    @classmethod
    def load(cls, path, device=None):
        from .utils.checkpoint import load_checkpoint

        ck = load_checkpoint(path)
        cfg = KMeansConfig.from_dict(ck["config"])
        km = cls.from_config(cfg)
        dev = _default_device(device)
        km.cluster_centers_ = ck["centers"].to(dev)
        km.n_iter_ = int(ck["iteration"])
        km.history_ = ck.get("history", [])
        km.n_features_in_ = km.cluster_centers_.shape[1]
        return km


def _splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


def _step_generator(seed: int, rank: int, step: int) -> torch.Generator:
    """CPU generator for one mini-batch step (step -1: the init sample), keyed by
    (seed, rank, step) so a resumed fit draws the rows the uninterrupted one would."""
    key = _splitmix64(_splitmix64(_splitmix64(seed & 0xFFFFFFFFFFFFFFFF) ^ rank) ^ (step & 0xFFFFFFFFFFFFFFFF))
    return torch.Generator(device="cpu").manual_seed(key & 0x7FFFFFFFFFFFFFFF)


class MiniBatchKMeans(_Serving):
    """Mini-batch k-means (Sculley 2010) over tensors or device-generated streams."""

    def __init__(self, n_clusters: int = 8, *, batch_size: int = 1024, max_iter: int = 100,
                 max_steps: int | None = None, init="k-means++", init_size: int | None = None,
                 dtype="float32", device=None, seed: int = 0, comm: Comm | None = None, frozen=None,
                 tol: float = 0.0, verbose: int = 0, init_sampling: str = "exact"):
        self.n_clusters = int(n_clusters)
        self.batch_size = int(batch_size)
        if init_sampling not in ("exact", "two-stage"):
            raise ValueError(f"init_sampling must be 'exact' or 'two-stage', got {init_sampling!r}")
        self.init_sampling = init_sampling
        self.max_iter = int(max_iter)
        self.max_steps = max_steps
        self.init = init
        self.init_size = init_size
        self.dtype = resolve_dtype(dtype)
        self.device = device
        self.seed = int(seed)
        self.comm = comm
        self.frozen = frozen
        self.tol = float(tol)
        self.verbose = verbose
        self._eng = None

    def _engine(self, D, device):
        if self._eng is None:
            comm = self.comm or get_comm()
            self._eng = MiniBatchEngine(self.n_clusters, D, self.batch_size, dtype=self.dtype,
                                        device=device, comm=comm, frozen=self.frozen)
        return self._eng

    def _init_centers(self, sample: torch.Tensor):
        comm = self.comm or get_comm()
        D = sample.shape[1]
        n_global, start = _shard_info(sample.shape[0], comm, sample.device)
        Xs = pad_columns(sample) if sample.is_cuda else sample
        return resolve_init(self.init, Xs, D, self.n_clusters, n_global, start, comm, self.seed,
                            None, sampling=self.init_sampling)[:, :D]

    def fit(self, X, *, resume_from=None, checkpoint_every: int = 0, checkpoint_dir=None):
        """Fit on a tensor/array (random batches each step; ``max_iter`` epochs).

        Batch row j of step s on rank r is local row floor(u * n) for a Philox draw keyed by
        (seed; j, s, r) (:mod:`mikmeans.data.sampler`), so the sampler's state is the step
        counter itself: ``checkpoint_every`` saves centres, running counts, scales and the
        step, and ``resume_from`` continues such a run with the rows every later step draws
        -- bit for bit the uninterrupted fit on the same world size.

        On a GPU the memory plan (``memory_plan_``, parallel/memplan.py) keeps the shard in
        HBM when it fits and draws every batch on the device (csrc/rows.hip: one gather
        kernel, no host work per step); a shard over the budget stays in host memory and its
        batches (the same rows) are gathered on the host.  The fixed-point scales come from
        the whole shard's column maxima, so no batch can saturate them and steps never
        synchronise with the host (the ``tol`` check reads the shift every 10 steps)."""
        from .data.sampler import sample_indices
        from .ops import col_stats
        from .parallel import memplan
        from .utils import faults
        from .utils.checkpoint import load_checkpoint

        comm = self.comm or get_comm()
        device = _default_device(self.device, X) if self.device is not None or comm.world == 1 else comm.device
        if not torch.is_tensor(X):
            a = np.asarray(X)
            X = torch.from_numpy(np.ascontiguousarray(a if a.dtype in (np.float32, np.float64)
                                                      else a.astype(np.float32)))
            self._numpy_io = True
        else:
            self._numpy_io = False
        n, D = int(X.shape[0]), int(X.shape[1])
        gpu = device.type == "cuda" and native_dpad(D, self.dtype) != 0
        b = min(self.batch_size, n) if n else 0
        self.memory_plan_ = None
        resident = True
        if gpu:
            x_ready = (torch.is_tensor(X) and X.device == device and X.dtype == self.dtype
                       and (not n or pad_columns(X[:0]).data_ptr() == X[:0].data_ptr()))
            src_es = X.element_size() if torch.is_tensor(X) else 4
            plan = memplan.plan_minibatch(n, D, self.n_clusters, self.dtype, batch_rows=self.batch_size,
                                          resident=True, init_rows=self.init_size, copy_x=not x_ready,
                                          src_itemsize=src_es if not X.is_cuda else memplan.esize_of(self.dtype))
            plan.budget = memplan.hbm_budget(device)
            if not plan.fits and not X.is_cuda:
                plan = memplan.plan_minibatch(n, D, self.n_clusters, self.dtype, batch_rows=self.batch_size,
                                              resident=False, init_rows=self.init_size, src_itemsize=src_es)
                plan.budget = memplan.hbm_budget(device)
                resident = False
            if not plan.fits:
                raise memplan.HBMCapacityError(f"MiniBatchKMeans.fit: {plan.summary()} does not fit; "
                                               "use a smaller batch_size or more ranks")
            self.memory_plan_ = plan.as_dict()
        # (sizes only: the fit's device copies are freed when it returns; a refit allocates
        # its own before anything of this one could still be referenced)
        self._fit_buffer_bytes = {}
        if not gpu or resident:
            Xt = _device_rows(X, device, self.dtype, gpu)
            Xh = None
        else:
            Xt, Xh = None, (X if X.device.type == "cpu" else X.cpu())
        eng = self._engine(D, device)
        if eng.gpu:
            # per-column bound of the whole shard (in the compute dtype): fixed scales, never exceeded
            if Xt is not None:
                bound = col_stats(Xt, stats=False).absmax
            else:
                bound = torch.zeros(D, dtype=torch.float64)
                for i in range(0, n, 1 << 20):
                    xb = Xh[i : i + (1 << 20)].to(self.dtype).float().abs()
                    bound = torch.maximum(bound, xb.amax(0).double())
            eng.set_bound(bound)
        # the fit's own device buffers, allocated before the seeding so the plan's phases
        # (persistent + the largest transient) bound the real peak
        from .parallel.memplan import _r

        buf = rows = None
        fb = self._fit_buffer_bytes
        if eng.gpu and Xt is not None and Xt.data_ptr() != getattr(X, "data_ptr", lambda: None)():
            fb["X"] = _r(Xt.numel() * Xt.element_size())     # the fit's device copy of the shard
        if eng.gpu and b:
            if Xt is not None:    # device shard: the step reads X[rows] in place, nothing gathered
                rows = torch.empty(b, dtype=torch.int64, device=device)
                fb["rows"] = _r(rows.numel() * rows.element_size())
            else:                 # host shard: the batch's rows are gathered on the host
                buf = torch.zeros((b, eng.Dp), dtype=self.dtype, device=device)
                fb["batch"] = _r(buf.numel() * buf.element_size())
        if resume_from is not None:
            ck = load_checkpoint(resume_from, comm=comm)
            if ck.get("kind") != "minibatch" or int(ck["n_features"]) != D:
                raise ValueError(f"{resume_from} is not a mini-batch checkpoint for {D} features")
            shard_bound = eng.bound.clone() if (eng.gpu and eng.bound is not None) else None
            eng.load_state(ck["centers"], ck["tensors"], ck["iteration"], ck.get("rescales", 0))
            if shard_bound is not None and eng.bound is not None:
                # the restored scales must still cover this shard (the fit's M-step runs
                # unclamped): a checkpoint written with a smaller bound (fit_stream's, or an
                # earlier fit's first-batch bound) is widened to the shard's (all-reduced MAX)
                eng.set_bound(torch.maximum(eng.bound.to(shard_bound.device), shard_bound))
        else:
            g = _step_generator(self.seed, comm.rank, -1)
            init_n = min(n, self.init_size or max(3 * self.batch_size, 3 * self.n_clusters))
            sample_idx = torch.randperm(n, generator=g)[:init_n]
            sample = (Xt[sample_idx.to(Xt.device)] if Xt is not None
                      else _device_rows(Xh[sample_idx], device, self.dtype, True))
            eng.set_centers(self._init_centers(sample))
            del sample                         # (the plan's "init" phase: freed before the steps)
            eng.steps = 0
        # the step count must be the same on every rank (each step is a collective): derive
        # it from the global row count, never from this rank's shard size
        n_global, _ = _shard_info(n, comm, comm.device)
        steps = self.max_steps or max(1, math.ceil(self.max_iter * n_global / (self.batch_size * comm.world)))
        C = native_mod() if eng.gpu else None
        while eng.steps < steps:
            s = eng.steps
            if not n:
                eng.partial_fit(X[:0].to(device) if not eng.gpu else buf_empty(eng, device))
            elif rows is not None:
                C.sample_index(n, b, self.seed, comm.rank, s, rows)           # Philox draws on device
                eng.partial_fit_rows(Xt, rows)
            else:
                idx = torch.from_numpy(sample_indices(n, b, self.seed, comm.rank, s))
                if eng.gpu:
                    buf[:, :D].copy_(Xh[idx].to(device, non_blocking=False))
                    eng.partial_fit(buf)
                else:
                    eng.partial_fit(Xt[idx])
            faults.maybe_fail(comm.rank, eng.steps)
            if checkpoint_every and checkpoint_dir and eng.steps % checkpoint_every == 0:
                self._finish(eng)
                self._save(checkpoint_dir, comm)
            if self.tol > 0 and (s + 1) % 10 == 0:
                if float(eng.shift.sum()) <= self.tol:
                    break
        self._finish(eng)
        if Xt is not None:
            self.labels_ = self.predict(Xt)
        else:   # host shard: label it in batch-sized blocks (memplan.plan_minibatch "predict")
            self.labels_ = self._assign_rows(Xh, False, block_rows=max(1, b))[0]
        if self._numpy_io and torch.is_tensor(self.labels_):
            self.labels_ = self.labels_.cpu().numpy()
        return self

    def fit_stream(self, stream, steps: int, init_batch: torch.Tensor | None = None, *, resume_from=None,
                   checkpoint_every: int = 0, checkpoint_dir=None):
        """Fit on an iterator of per-rank batches (e.g. :class:`~mikmeans.data.blobs.BlobStream`).

        ``steps`` counts the whole run; with ``checkpoint_every`` the state (centres, running
        counts, fixed-point scales, step and the stream's global row position) is saved
        every that many steps, and ``resume_from`` continues such a run -- also on another
        world size: a stream with the same global batch (``batch * world``) then replays the
        same rows per step and the exact integer M-step gives the same centres (the
        reference's export/import of the whole board, app.mjs:263-282).  Across world sizes
        that holds up to near-ties of the bf16 assign: its key offset is shared by a
        workgroup of rows, and which rows share one changes with the per-rank batch
        (f32 data, and a resume on the same world size, are bitwise).  A generic iterator
        must itself be positioned at the checkpoint's ``stream_pos`` (BlobStream is seeked)."""
        from .utils import faults
        from .utils.checkpoint import load_checkpoint

        comm = self.comm or get_comm()
        if resume_from is not None:
            ck = load_checkpoint(resume_from, comm=comm)
            if ck.get("kind") != "minibatch":
                raise ValueError(f"{resume_from} is not a mini-batch checkpoint")
            device = torch.device(getattr(stream, "device", None) or self.device or comm.device)
            eng = self._engine(int(ck["n_features"]), device)
            eng.load_state(ck["centers"], ck["tensors"], ck["iteration"], ck.get("rescales", 0))
            if hasattr(stream, "seek"):
                stream.seek(int(ck["stream_pos"]))
        else:
            first = init_batch if init_batch is not None else next(iter(stream))
            eng = self._engine(first.shape[1], first.device)
            eng.set_centers(self._init_centers(first.to(self.dtype)))
        vb = getattr(stream, "value_bound", None)
        if vb is not None and eng.gpu and (eng.col_exp is None or bool((eng.bound >= float(vb)).all())):
            # bounded stream: no per-step clamp check (also after a resume, whose restored
            # scales came from the same bound)
            eng.value_bound = float(vb)
            eng.bounded = True
        while eng.steps < steps:
            Xb = next(stream)
            eng.partial_fit(Xb, getattr(stream, "last_norms", None))
            faults.maybe_fail(comm.rank, eng.steps)
            if checkpoint_every and checkpoint_dir and eng.steps % checkpoint_every == 0:
                self._finish(eng)
                self._save(checkpoint_dir, comm, stream_pos=stream.position() if hasattr(stream, "position")
                           else None)
        self._finish(eng)
        return self

    # ------------------------------------------------------------- persist
    def _save(self, path, comm, stream_pos=None):
        from .utils.checkpoint import save_checkpoint

        eng = self._eng
        cfg = {"n_clusters": self.n_clusters, "batch_size": self.batch_size, "max_iter": self.max_iter,
               "init": self.init if isinstance(self.init, str) else "array", "dtype": str(self.dtype),
               "seed": self.seed, "tol": self.tol}
        extra = {"kind": "minibatch", "rescales": getattr(eng, "rescales", 0),
                 # the samplers are counter-based: (seed, rank, step) is the whole RNG state
                 "rng": {"scheme": "fit: Philox4x32-10 row draws keyed by (seed; row, step, rank), "
                                   "data/sampler.py; streams: Philox4x32-10 by global row (BlobStream)",
                         "seed": self.seed, "step": int(eng.steps)}}
        if stream_pos is not None:
            extra["stream_pos"] = int(stream_pos)
        return save_checkpoint(path, eng.centers, eng.steps, cfg, comm=comm, extra=extra,
                               tensors=eng.state_tensors())

    def save(self, path):
        """Checkpoint the fitted state (centres, running counts, scales, step count)."""
        self._check_fitted()
        return self._save(path, self.comm or get_comm())

    @classmethod
    def load(cls, path, device=None, comm=None):
        """A MiniBatchKMeans that continues from ``path`` (``partial_fit`` / ``predict``)."""
        from .config import resolve_dtype
        from .utils.checkpoint import load_checkpoint

        ck = load_checkpoint(path, comm=comm)
        if ck.get("kind") != "minibatch":
            raise ValueError(f"{path} is not a mini-batch checkpoint")
        c = ck["config"]
        dt = "bfloat16" if "bfloat16" in c.get("dtype", "") else "float32"
        km = cls(c["n_clusters"], batch_size=c["batch_size"], max_iter=c.get("max_iter", 100),
                 init=c.get("init", "k-means++"), dtype=resolve_dtype(dt), device=device,
                 seed=c.get("seed", 0), comm=comm, tol=c.get("tol", 0.0))
        dev = _default_device(device)
        eng = km._engine(int(ck["n_features"]), dev)
        eng.load_state(ck["centers"], ck["tensors"], ck["iteration"], ck.get("rescales", 0))
        km._finish(eng)
        return km

    def partial_fit(self, Xb):
        comm = self.comm or get_comm()
        device = _default_device(self.device, Xb) if self.device is not None or comm.world == 1 else comm.device
        Xt, _ = _to_tensor(Xb, device, self.dtype)
        eng = self._engine(Xt.shape[1], device)
        if not hasattr(self, "cluster_centers_"):
            eng.set_centers(self._init_centers(Xt))
        eng.partial_fit(Xt)
        self._finish(eng)
        return self

    def device_buffers(self) -> dict:
        """Allocator bytes of the last ``fit``'s persistent device buffers (engine + the fit's
        shard copy / row list / batch buffer), named as ``memplan.plan_minibatch`` plans them."""
        out = dict(self._eng.device_buffers()) if self._eng is not None else {}
        out.update(getattr(self, "_fit_buffer_bytes", {}))
        return out

    def _finish(self, eng):
        self.cluster_centers_ = eng.centers.clone()
        self.n_steps_ = eng.steps
        self.counts_ = eng.vcount.clone()

    def predict(self, X):
        self._check_fitted()
        labels, _, was_numpy = self._assign_rows(X, False)
        return labels.cpu().numpy() if was_numpy else labels

    def fit_predict(self, X):
        return self.fit(X).predict(X)

    def score(self, X):
        self._check_fitted()
        _, mind, _ = self._assign_rows(X, True)
        return -float(mind.sum(dtype=torch.float64))


# ------------------------------------------------------------------ functional
def fit(X, k: int, **kw):
    """``fit(X, k) -> (centers, labels)`` — the north-star functional surface."""
    km = KMeans(n_clusters=k, **kw).fit(X)
    return km._out(km.cluster_centers_), km._out(km.labels_)


def _given_centers(X, centers, dtype):
    """The functional entry points' inputs: ``(Xt, c, was_numpy)``, the float32 centres on their
    own device (the default device for array-likes) and ``X`` on it in ``dtype``."""
    c = torch.as_tensor(np.asarray(centers) if not torch.is_tensor(centers) else centers, dtype=torch.float32)
    dev = c.device if torch.is_tensor(centers) else _default_device(None)
    Xt, was_numpy = _to_tensor(X, dev, resolve_dtype(dtype))
    return Xt, c.to(dev), was_numpy


def predict(X, centers, dtype="float32"):
    """Nearest-centre labels of ``X`` for given ``centers``."""
    Xt, c, was_numpy = _given_centers(X, centers, dtype)
    labels, _ = ops.assign(Xt, c, with_dist=False)
    return labels.cpu().numpy() if was_numpy else labels


def predict_topk(X, centers, m: int, dtype="float32"):
    """The ``m`` nearest of the given ``centers`` for every row of ``X``: ``(labels [n, m],
    Euclidean distances [n, m])``, nearest first (``KMeans.predict_topk`` without a model)."""
    Xt, c, was_numpy = _given_centers(X, centers, dtype)
    idx, d2 = ops.topk(Xt, c, m)
    d = d2.sqrt()
    return (idx.cpu().numpy(), d.cpu().numpy()) if was_numpy else (idx, d)


def cluster_report(X, centers, dtype="float32") -> ClusterReport:
    """Per-cluster quality of ``X`` under the given ``centers``
    (``KMeans.cluster_report`` without a model; with a process group ``X`` is the rank's shard)."""
    Xt, c, was_numpy = _given_centers(X, centers, dtype)
    rep = _report_table(c, get_comm(), resolve_dtype(dtype), lambda table: ops.quality_rows(table, Xt, c))
    return rep.numpy() if was_numpy else rep


def cluster_exemplars(X, centers, m: int, dtype="float32", farthest: bool = False):
    """For each of the given ``centers`` the ``m`` rows of ``X`` nearest it (``farthest``: farthest
    from it) among the rows assigned to it: ``(rows [K, m], Euclidean distances [K, m])``
    (``KMeans.cluster_exemplars`` without a model; with a process group ``X`` is the rank's shard
    and the rows are global indices)."""
    Xt, c, was_numpy = _given_centers(X, centers, dtype)
    rows, d = _exemplar_lists(c.shape[0], m, c.device, get_comm(), Xt.shape[0], farthest, False,
                              lambda table: ops.exemplar_rows(table, Xt, c, farthest=farthest))
    return (rows.cpu().numpy(), d.cpu().numpy()) if was_numpy else (rows, d)


def cluster_quantiles(X, centers, q, dtype="float32"):
    """Exact per-cluster quantiles of the Euclidean distances of the rows of ``X`` to the nearest
    of the given ``centers``: ``(values [K, Q], counts [K])`` (``KMeans.cluster_quantiles`` without
    a model; with a process group ``X`` is the rank's shard)."""
    Xt, c, was_numpy = _given_centers(X, centers, dtype)
    v, counts = ops.cluster_quantiles(Xt, c, q, reduce=_allreduce(get_comm()))
    v = v.sqrt()
    return (v.cpu().numpy(), counts.cpu().numpy()) if was_numpy else (v, counts)


class _GivenCenters(_Serving):
    """The serving surface over given centres (the functional entry points that need a model)."""

    def __init__(self, centers: torch.Tensor, dtype):
        self.cluster_centers_, self.dtype = centers, dtype


def build_index(X, centers, dtype="float32") -> ClusterIndex:
    """Index the rows of ``X`` by the nearest of the given ``centers`` (``KMeans.build_index``
    without a model; with a process group ``X`` is the rank's shard and the rows are global
    indices)."""
    c = torch.as_tensor(np.asarray(centers) if not torch.is_tensor(centers) else centers, dtype=torch.float32)
    dev = c.device if torch.is_tensor(centers) else _default_device(None)
    return _GivenCenters(c.to(dev), resolve_dtype(dtype)).build_index(X)


def build_pq_index(X, centers, n_subvectors: int = 16, dtype="float32", **kw) -> PQIndex:
    """Index the rows of ``X`` under the given ``centers`` as ``n_subvectors`` one-byte codes a row
    (``KMeans.build_pq_index`` without a model, which takes the other arguments)."""
    c = torch.as_tensor(np.asarray(centers) if not torch.is_tensor(centers) else centers, dtype=torch.float32)
    dev = c.device if torch.is_tensor(centers) else _default_device(None)
    return _GivenCenters(c.to(dev), resolve_dtype(dtype)).build_pq_index(X, n_subvectors, **kw)


def fit_predict(X, k: int, **kw):
    return fit(X, k, **kw)[1]


def kmeans_plusplus(X, n_clusters: int, *, seed: int = 0, n_local_trials=None, comm: Comm | None = None,
                    dtype="float32", device=None, sampling: str = "exact"):
    """k-means++ seeding only; returns the ``[K, D]`` initial centres."""
    comm = comm or get_comm()
    dev = _default_device(device, X)
    Xt, was_numpy = _to_tensor(X, dev, resolve_dtype(dtype))
    D = Xt.shape[1]
    Xp = pad_columns(Xt) if Xt.is_cuda else Xt
    n_global, start = _shard_info(Xt.shape[0], comm, dev)
    name = "greedy-k-means++" if (n_local_trials or 1) > 1 else "k-means++"
    c = resolve_init(name, Xp, D, n_clusters, n_global, start, comm, seed, n_local_trials, sampling=sampling)
    return c.cpu().numpy() if was_numpy else c
