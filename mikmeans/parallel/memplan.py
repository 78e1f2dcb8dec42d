"""HBM-aware memory planning for MI355X (288 GB HBM3E per GPU) from the engines' real
allocations.

Every device buffer the fit engines allocate is listed here by name with its exact size
(rounded to the caching allocator's 512-byte granule), computed from the same launch
geometry the kernels use (a Python mirror of ``csrc/plan.h``, pinned against the native
functions by ``tests/test_memplan.py``).  :func:`plan_fit` turns (rows per rank, D, K,
dtype, options) and a byte budget into one of

* ``resident``  -- the rank's shard lives in HBM (:class:`~mikmeans.models.lloyd.LloydEngine`);
* ``streaming`` -- the shard stays in host memory and streams through two device chunk
  buffers every iteration (:class:`~mikmeans.models.streaming.StreamingLloydEngine`), with
  the largest chunk that fits;

or raises :class:`HBMCapacityError` when even the per-row state of a streamed fit (labels,
row norms: 8 B per row) does not fit -- a clear error instead of an allocator OOM half-way
through a fit, as the reference refuses its one capacity limit up front ("at most 3
centroids", app.mjs:127).  :func:`plan_minibatch` sizes a mini-batch fit (device-resident
shard + sampled batch, or a host shard gathered batch by batch).

The budget is ``MIKMEANS_HBM_BYTES`` when set (bytes this fit may allocate), else the
device's free memory plus what the caching allocator holds unused, minus headroom for the
runtime and RCCL (:func:`hbm_budget`).
"""
from __future__ import annotations

import math
import os
from dataclasses import asdict, dataclass, field

HBM_BYTES = 288 * 10**9          # MI355X HBM3E per GPU (spec)
GRANULE = 512                    # torch caching allocator rounding of every block
ROW_ALIGN = 1536                 # parallel/shard.py: shard / chunk row grid
SPLIT_MAX_ROWS = 1 << 18         # ops.SPLIT_MAX_ROWS: small batches keep u64 split keys
NSLOT, SLOT_STRIDE = 256, 8      # csrc/kernels.h
WDOT_SCRATCH = 1024              # csrc/rows.hip WDOT_BLOCKS (weighted-inertia partials)
COMPACT_ROWS = 4096              # csrc/rows.hip CMP_ROWS (candidate compaction block)
STAGING_BYTES = 1 << 26          # api._device_rows: host rows cross in blocks of this size
UPD_LDS_MAX = 160 * 1024         # csrc/plan.h
KS_NT = 1024
KS_LIST_BYTES = 2 * (KS_NT // 64) * 64 * 4


class HBMCapacityError(MemoryError):
    """The requested fit cannot be placed in the GPU's HBM budget in any supported mode."""


def _r(nbytes: int) -> int:
    """Bytes one allocation of ``nbytes`` takes from the caching allocator."""
    nbytes = int(nbytes)
    return 0 if nbytes <= 0 else -(-nbytes // GRANULE) * GRANULE


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


# ----------------------------------------------------------------- csrc/plan.h mirror
def esize_of(dtype) -> int:
    s = str(dtype)
    return 2 if "bfloat16" in s or s in ("bf16", "2") else 4


def vec_elems(esize: int) -> int:
    return 16 // esize


def padded_cols(D: int, esize: int) -> int:
    """ops.pad_columns: columns rounded up to a 16-byte multiple."""
    v = vec_elems(esize)
    return _cdiv(D, v) * v


def dpad_for(D: int, esize: int) -> int:
    """csrc/plan.h assign_dpad: powers of two up to 256, then 384 / 512 / 768 / 1024."""
    d = 4 * vec_elems(esize)
    while d < D and d < 256:
        d *= 2
    if D <= d:
        return d
    return next((w for w in (384, 512, 768, 1024) if D <= w), 0)


def upd_lds_bytes(K: int, ldc: int, weighted: bool) -> int:
    b = (K + 1) * ldc * 8 + (K + 1) * 4 + 8
    b = (b + 7) & ~7
    b += (K + 1) * 8 if weighted else 0
    return b + ((K + 1) * 2 + 7) // 8 * 8


def choose_sw(esize: int, K: int, D: int, weighted: bool, max_sw: int = 0) -> tuple[int, int]:
    """(slice width, LDS cell stride) of the column-slice M-step; (0, 0) = global fallback."""
    if K < 1 or D < 1 or (D * esize) % 4 or D % 2:
        return 0, 0
    dp = 2
    while dp < D:
        dp *= 2
    for sw in (64, 32, 16, 8, 4, 2):
        if sw > dp or (max_sw and sw > max_sw):
            continue
        if upd_lds_bytes(K, sw // 2 + 1, weighted) <= UPD_LDS_MAX:
            return sw, sw // 2 + 1
        if upd_lds_bytes(K, sw // 2, weighted) <= UPD_LDS_MAX:
            return sw, sw // 2
    return 0, 0


def n_chunks_slice(sw: int, D: int, N: int) -> int:
    if sw == 0:
        return 1
    n_slices = _cdiv(D, sw)
    nc = _cdiv(256, n_slices)
    nc = _cdiv(nc, 8) * 8
    if _cdiv(N, nc) < 256:
        nc = max(8, _cdiv(_cdiv(N, 256), 8) * 8)
    return nc


def choose_ks(esize: int, K: int, D: int):
    """K-split M-step plan (ks, kq, lpr, ldc) or None (plan::choose_ks)."""
    if K < 2 or D < 2 or D % 2 or (D * esize) % 4:
        return None
    v = 16 // esize
    lpr = 1
    while lpr * v < D:
        lpr *= 2
    if lpr > 64 or lpr < 8:
        return None
    ldc = lpr * v // 2 + 1
    ks = lpr // 4 if lpr // 4 > 1 else 1
    while ks > K:
        ks //= 2
    while True:
        kq = _cdiv(K, ks)
        if kq * ldc * 8 + kq * 4 + 16 + KS_LIST_BYTES <= UPD_LDS_MAX:
            return None if ks < 2 else (ks, kq, lpr, ldc)
        if ks >= 64:
            return None
        ks *= 2


def update_n_chunks(esize: int, K: int, D: int, N: int, weighted: bool) -> int:
    """update.hip update_n_chunks: M-step row chunks (slab depth) for an N-row pass."""
    sw = choose_sw(esize, K, D, weighted)[0]
    nc = n_chunks_slice(sw, D, N)
    if not weighted:
        ssw = choose_sw(esize, K, D, False)[0]
        ks = choose_ks(esize, K, D) if (0 < ssw < D and ssw * esize < 128) else None
        if ks is not None:
            nc = max(_cdiv(_cdiv(256, ks[0]), 8) * 8, nc)
    return nc


def assign_kpad(esize: int, dpad: int, K: int) -> int:
    ok = dpad >= 4 * vec_elems(esize) and dpad_for(dpad, esize) == dpad
    if not ok or K < 1 or K > (1 << 24):
        return 0
    ct = 1 if 16 * dpad * esize >= 16384 else 16384 // (16 * dpad * esize)
    m = 16 * ct
    return _cdiv(K, m) * m


def assign_cn_len(kpad: int) -> int:
    return _cdiv(kpad, 256) * 256


def staging_items(n: int, D: int, src_es: int, es: int, prefix: str) -> dict:
    """api._device_rows moving host rows to the device: one block at a time lands in its
    source dtype (and, when the destination rows are padded, converted to a contiguous
    block before the strided copy)."""
    if n <= 0:
        return {}
    rows = min(n, max(1, STAGING_BYTES // max(1, D * max(src_es, es))))
    it = {f"{prefix}_staging": _r(rows * D * src_es)}
    if padded_cols(D, es) != D and src_es != es:
        it[f"{prefix}_staging_cast"] = _r(rows * D * es)
    return it


# ------------------------------------------------------------------ inventories
def _centroid_items(K: int, Dp: int, esize: int, with_vcount: bool = False) -> dict:
    dpad = dpad_for(Dp, esize)
    kpad = assign_kpad(esize, dpad, K)
    it = {
        "C": _r(K * Dp * 4), "Cnew": _r(K * Dp * 4), "shift": _r(K * 4), "counts": _r(K * 4),
        "pack": _r(kpad * dpad * esize), "cn": _r(assign_cn_len(kpad) * 4),
        "slots": _r(NSLOT * SLOT_STRIDE * 8),
    }
    if with_vcount:
        it["vcount"] = _r(K * 8)
    return it


def kpp_workspace(n: int, Dp: int, K: int, trials: int = 1, prune: bool = True) -> dict:
    """models/init.py _kpp_gpu + init_kmeanspp device buffers (freed after seeding)."""
    rpb = max(256, _cdiv(n, 2048)) if n else 256
    nb = max(1, _cdiv(n, rpb))
    it = {"kpp_centers": _r(K * Dp * 4), "kpp_u": _r(max(0, K - 1) * trials * 8),
          "kpp_d2": _r(max(n, 1) * 4), "kpp_block_sums": _r(nb * 8), "kpp_cand": _r(trials * Dp * 4)}
    if prune:
        it["kpp_owner"] = _r(max(n, 1) * 4)
        it["kpp_cc"] = _r(K * 4)
    if trials > 1:
        it["kpp_d2c"] = _r(max(n, 1) * 4)
        it["kpp_bsc"] = _r(nb * 8)
        it["kpp_pots"] = _r(trials * 8)
    return it


def _init_items(init, n: int, Dp: int, D: int, K: int, trials: int) -> dict:
    name = init.lower().replace("_", "-") if isinstance(init, str) else "array"
    if name in ("k-means++", "kmeans++", "kpp", "greedy-k-means++", "greedy-kmeans++"):
        t = trials if trials else (2 + int(math.log(K)) if name.startswith("greedy") and K > 1 else 1)
        return kpp_workspace(n, Dp, K, max(1, t))
    if name in ("k-means||", "kmeans||", "scalable-k-means++"):
        # models/init.py init_kmeans_parallel: d2, flags, compacted rows, row norms, and the
        # nearest-candidate pass (best distance, int64 labels, one launch's labels / distances)
        m = 5 * 2 * K + 1
        return {"kpar_d2": _r(n * 4), "kpar_cand": _r(n), "kpar_rows": _r(n * 8), "kpar_xn": _r(n * 4),
                "kpar_best": _r(n * 4), "kpar_labels": _r(n * 8), "kpar_launch": 2 * _r(n * 4),
                "kpar_candidates": _r(m * D * 8), "kpar_scratch": _r(max(1, -(-n // COMPACT_ROWS)) * 8)}
    return {"init_rows": _r(K * D * 8)}


@dataclass
class MemoryPlan:
    mode: str                   # resident | streaming | minibatch-resident | minibatch-host
    n: int                      # rows of this rank
    D: int
    Dp: int                     # stored (16-byte padded) columns
    K: int
    dtype: str
    persistent: dict = field(default_factory=dict)   # live for the whole fit
    transient: dict = field(default_factory=dict)    # phases: the largest one counts
    budget: int | None = None
    chunk_rows: int = 0
    batch_rows: int = 0

    @property
    def persistent_bytes(self) -> int:
        return sum(self.persistent.values())

    @property
    def transient_bytes(self) -> int:
        return max((sum(v.values()) for v in self.transient.values()), default=0)

    @property
    def peak(self) -> int:
        return self.persistent_bytes + self.transient_bytes

    @property
    def fits(self) -> bool:
        return self.budget is None or self.peak <= self.budget

    def as_dict(self) -> dict:
        d = asdict(self)
        d.update(peak=self.peak, persistent_bytes=self.persistent_bytes,
                 transient_bytes=self.transient_bytes, fits=self.fits)
        return d

    def summary(self) -> str:
        gb = 1e9
        s = (f"{self.mode}: n={self.n} D={self.D} K={self.K} {self.dtype} peak {self.peak / gb:.3f} GB"
             + (f" of {self.budget / gb:.3f} GB budget" if self.budget is not None else ""))
        if self.chunk_rows:
            s += f", chunks of {self.chunk_rows} rows"
        if self.batch_rows:
            s += f", batches of {self.batch_rows} rows"
        return s


COLSTAT_BLOCKS = 8192     # csrc/finalize.hip


def colstat_cap(Dp: int) -> int:
    """csrc/finalize.hip ``colstat_cap``: blocks keeping the f64 partials within 32 MiB, 2048..8192."""
    return max(2048, min(COLSTAT_BLOCKS, (32 << 20) // (24 * max(Dp, 1))))


def colstat_rows(es: int, n: int, Dp: int) -> int:
    """Rows of the column-statistics partials one setup pass over ``n`` rows writes
    (csrc/finalize.hip ``colstat_rows``): its widest launch's block count."""
    V = 16 // es
    npt, rows = Dp // V, 0
    for p0 in range(0, npt, 64):
        L = 1
        while L < min(64, npt - p0):
            L *= 2
        rows = max(rows, min(colstat_cap(Dp), -(-n // (256 // L))))
    return rows


def _setup_items(n: int, Dp: int, es: int) -> dict:
    """The setup pass's transient (LloydEngine / StreamingLloydEngine ``col_stats``): the
    per-block f64 partials of the column statistics, zeroed and reduced in a fixed order."""
    return {"colstat_part": _r(colstat_rows(es, n, Dp) * 3 * Dp * 8)} if n else {}


GSTATS_ROWS = 256   # csrc/kernels.h: rows per group of the assign's per-group seed statistics


def group_stats_bytes(n: int, Dp: int, es: int) -> int:
    """Bytes of the full assign's per-group seed statistics (ops.CentroidPack.group_stats): an f32
    pair per 256-row group, for bf16 rows of 65..128 padded features; 0 where no kernel reads them."""
    if es != 2 or dpad_for(Dp, es) != 128 or n <= 0:
        return 0
    return _cdiv(n, GSTATS_ROWS) * 8


def plan_resident(n: int, D: int, K: int, dtype="bfloat16", *, weighted: bool = False,
                  incremental: bool = True, init="k-means++", n_local_trials: int | None = None,
                  copy_x: bool = True, empty_policy: str = "keep", bounded: bool = False,
                  src_itemsize: int | None = None) -> MemoryPlan:
    """Device-resident Lloyd fit of an ``n``-row shard (``KMeans.fit``): the engine's buffers
    (models/lloyd.py ``LloydEngine._init_gpu``), the seeding workspace and the final E-step.
    ``bounded``: the Hamerly E-step's per-row bounds, flags and compacted rows (17 B/row; bf16
    adds the rows' seed offsets, 4 B/row)."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    wted = weighted
    p: dict = {}
    if copy_x:
        p["X"] = _r(n * Dp * es)
    if weighted:
        p["weights"] = _r(n * 4)
    p["labels"] = _r(n * 4)
    p["xn"] = _r(n * 4)
    if group_stats_bytes(n, Dp, es):
        p["gstats"] = _r(group_stats_bytes(n, Dp, es))   # the assign's per-group seed statistics, once per fit
    if weighted or empty_policy == "farthest":
        p["mind"] = _r(n * 4)          # written by every step's assign (relocation reads it)
    if weighted:
        p["wdot_scratch"] = _r(WDOT_SCRATCH * 8)
    nch = update_n_chunks(es, K, Dp, max(n, 1), wted or incremental)
    p["slab"] = _r(nch * K * Dp * 8)
    p["cnt_slab"] = _r(nch * K * 8)
    p["packed"] = _r((K * Dp + K + 2) * 8)
    p.update(_centroid_items(K, Dp, es))
    final = {"labels_out": _r(n * 4), "mind_out": _r(n * 4)}
    if 0 < n <= SPLIT_MAX_ROWS:
        if bounded:
            final["split_keys"] = _r(n * 8)   # (the bounded E-step's gathered passes take no keys)
        else:
            p["split_keys"] = _r(n * 8)
    if incremental and n and n < 2**31 and choose_sw(es, K, Dp, True)[0] > 0:
        cap = max(1, min(n, int(n * 0.125)))
        p.update(delta_prev=_r(n * 4), delta_list=_r(cap * 8), delta_count=_r(4),
                 delta_tot=_r((K * Dp + K) * 8))
    if bounded:
        p.update(bound_ub=_r(n * 4), bound_lb=_r(n * 4), bound_cand=_r(n), bound_rows=_r(n * 8),
                 bound_count=_r(8), bound_scratch=_r(max(1, -(-n // COMPACT_ROWS)) * 8), bound_work=_r(16),
                 bound_qshift=_r(K * 4))
        if es == 2 and n:
            p["bound_oseed"] = _r(n * 4)   # every row's full-pass seed offset (bf16 keys)
    tr = {"init": _init_items(init, n, Dp, D, K, n_local_trials or 0), "final_assign": final,
          "setup": _setup_items(n, Dp, es)}
    if copy_x and (src_itemsize or es) != es:
        tr["load"] = staging_items(n, D, src_itemsize or es, es, "x")
    return MemoryPlan("resident", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


def plan_streaming(n: int, D: int, K: int, dtype="bfloat16", *, chunk_rows: int, weighted: bool = False,
                   init="k-means++", n_local_trials: int | None = None, init_rows: int | None = None,
                   src_itemsize: int | None = None, empty_policy: str = "keep") -> MemoryPlan:
    """Out-of-core Lloyd (models/streaming.py): per-row labels / norms on the device, two
    chunk buffers (+ a staging buffer when the host rows need a dtype / padding change),
    the M-step slab of one chunk, the init sample and its seeding workspace."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    R = stream_chunk_rows(chunk_rows, n)
    p = {"labels": _r(n * 4), "xn": _r(n * 4)}
    if weighted:
        p["weights"] = _r(n * 4)
        p["wdot_scratch"] = _r(WDOT_SCRATCH * 8)
    if weighted or empty_policy == "farthest":
        p["mind"] = _r(n * 4)
    p["chunk_bufs"] = 2 * _r(R * Dp * es)
    sis = src_itemsize or es
    if sis != es or Dp != D:
        p["staging"] = 2 * _r(R * D * sis)
    nch = update_n_chunks(es, K, Dp, R, weighted)
    p["slab"] = _r(nch * K * Dp * 8)
    p["cnt_slab"] = _r(nch * K * 8)
    p["packed"] = 2 * _r((K * Dp + K + 2) * 8)
    p.update(_centroid_items(K, Dp, es))
    if 0 < R <= SPLIT_MAX_ROWS:
        p["split_keys"] = _r(R * 8)
    name = init.lower().replace("_", "-") if isinstance(init, str) else "array"
    if name in ("random", "array"):
        # (api.KMeans._init_centers: rows fetched from the host shard, no device sample)
        init_tr = _init_items(init, n, Dp, D, K, 0)
    else:   # k-means++ seeds on a device-resident init_size-row sample
        m = min(n, init_rows or max(20 * K, 1 << 16))
        init_tr = {"sample": _r(m * Dp * es), **_init_items(init, m, Dp, D, K, n_local_trials or 0)}
    tr = {"init": init_tr, "final_assign": {"labels_out": _r(n * 4), "mind_out": _r(n * 4)},
          "setup": _setup_items(min(R, n), Dp, es)}      # (the statistics pass, one chunk at a time)
    pl = MemoryPlan("streaming", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)
    pl.chunk_rows = R
    return pl


def stream_chunk_rows(chunk_rows: int, n: int) -> int:
    """StreamingLloydEngine's chunk: ``chunk_rows`` rounded up to the 1536-row grid, at most n."""
    return max(1, min(_cdiv(int(chunk_rows), ROW_ALIGN) * ROW_ALIGN, max(n, 1)))


def plan_minibatch(n: int, D: int, K: int, dtype="bfloat16", *, batch_rows: int, resident: bool = True,
                   init="k-means++", init_rows: int | None = None, copy_x: bool = True,
                   src_itemsize: int = 4) -> MemoryPlan:
    """Mini-batch fit (api.MiniBatchKMeans.fit, models/minibatch.py): the engine's buffers
    (``MiniBatchEngine.device_buffers``) plus the fit's own -- the shard itself when it is
    device-resident (each step then reads ``X[rows]`` in place through an int64 index list
    drawn on the device), or one gathered batch buffer for a host shard."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    b = int(batch_rows)
    p = {}
    if resident:
        if copy_x:
            p["X"] = _r(n * Dp * es)
        p["rows"] = _r(b * 8)
    else:
        p["batch"] = _r(b * Dp * es)
    p["batch_labels"] = _r(b * 4)
    p["clampc"] = _r(4)
    nch = update_n_chunks(es, K, Dp, b, False)
    p["slab"] = _r(nch * K * Dp * 8)
    p["cnt_slab"] = _r(nch * K * 8)
    p["packed"] = _r((K * Dp + K + 3) * 8)
    p.update(_centroid_items(K, Dp, es, with_vcount=True))
    if not resident and 0 < b <= SPLIT_MAX_ROWS:
        p["split_keys"] = _r(b * 8)     # (gathered batches take the one-pass grid: no keys)
    m = min(n, init_rows or max(3 * b, 3 * K))
    pred = {"labels_out": _r(n * 4)}
    if not resident and n:
        # api.MiniBatchKMeans.fit labels a host shard in batch-sized blocks
        # (_Serving._assign_rows): the block as copied (source dtype), its cast to the compute
        # dtype and padding, its labels
        B = min(n, max(1, b))
        pred["block_src"] = _r(B * D * src_itemsize)
        if src_itemsize != es:
            pred["block_cast"] = _r(B * D * es)
        if Dp != D:
            pred["block_padded"] = _r(B * Dp * es)
        pred["block_labels"] = _r(B * 4)
    init_tr = {"sample": _r(m * Dp * es), **_init_items(init, m, Dp, D, K, 0)}
    tr = {"init": init_tr, "predict": pred}
    if resident and copy_x and src_itemsize != es:
        tr["load"] = staging_items(n, D, src_itemsize, es, "x")
    if not resident:
        # the init sample crosses from the host through api._device_rows' staging block, and
        # every step's gathered host batch lands in its source dtype before the cast into
        # the batch buffer
        init_tr.update(staging_items(m, D, src_itemsize, es, "sample"))
        tr["step"] = {"batch_src": _r(b * D * src_itemsize)}
    pl = MemoryPlan("minibatch-resident" if resident else "minibatch-host", n, D, Dp, K,
                    "bfloat16" if es == 2 else "float32", p, tr)
    pl.batch_rows = b
    return pl


# ------------------------------------------------------------------------- index
TOPK_BLOCK_ROWS = 1 << 22        # ops.TOPK_BLOCK_ROWS: rows per top-1 pass
PT_MAX_BLOCKS, PT_MAX_CELLS = 1024, 1 << 20      # csrc/ivf.hip


def partition_blocks(n: int, K: int) -> int:
    """csrc/ivf.hip partition_blocks: workgroups (and count cells per label) of a partition."""
    cap = max(1, min(PT_MAX_BLOCKS, PT_MAX_CELLS // max(K, 1)))
    return max(1, min(_cdiv(n, 1024), cap))


def index_tiles(n: int, K: int) -> int:
    """ops.index_tiles: 16-row tiles of the row pack, every list padded to whole tiles."""
    return (n + 15 * K) // 16


def plan_index(n: int, D: int, K: int, dtype="bfloat16", *, block_rows: int | None = None) -> MemoryPlan:
    """An index of ``n`` rows (ops.index_build / KMeans.build_index): what it keeps -- the row pack
    (every list padded to whole 16-row tiles, rows padded to the kernels' width), its ``cn``,
    ``order`` and the two offset arrays -- and the build's scratch: every row's list and position,
    one block of top-1 output with its row norms, and the partition's count cells."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    cols = dpad_for(Dp, es) or Dp
    rows = index_tiles(n, K) * 16
    p = {"row_pack": _r(rows * cols * es), "cn": _r(rows * 4), "order": _r(n * 8), "offsets": _r((K + 1) * 8),
         "tile_offsets": _r((K + 1) * 8)}
    B = min(n, int(block_rows) if block_rows else TOPK_BLOCK_ROWS)
    tr = {"build": {"labels": _r(n * 4), "row_pos": _r(n * 8), "top1_idx": _r(B * 4), "top1_d2": _r(B * 4),
                    "top1_xn": _r(B * 4), "top1_labels": _r(B * 4), "partition_cells": _r(K * partition_blocks(n, K) * 8)}}
    return MemoryPlan("index", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


def plan_index_update(n_old: int, n_total: int, D: int, K: int, dtype="bfloat16", *,
                      block_rows: int | None = None) -> MemoryPlan:
    """An index of ``n_old`` ids updated to ``n_total`` (ops.index_add / ops.index_remove, which
    keeps ``n_total = n_old``): the old index and the new one, both alive while the rows are copied
    across, and the update's scratch -- every id's list and position in the new order, the old ids'
    lists and positions, one block of top-1 output over the new rows and the partition's count
    cells."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    cols = dpad_for(Dp, es) or Dp
    p = {}
    for tag, n in (("old_", n_old), ("", n_total)):
        rows = index_tiles(n, K) * 16
        p.update({tag + "row_pack": _r(rows * cols * es), tag + "cn": _r(rows * 4), tag + "order": _r(n * 8),
                  tag + "offsets": _r((K + 1) * 8), tag + "tile_offsets": _r((K + 1) * 8)})
    B = min(n_total - n_old, int(block_rows) if block_rows else TOPK_BLOCK_ROWS)
    tr = {"update": {"labels": _r(n_total * 4), "row_pos": _r(n_total * 8), "old_labels": _r(n_old * 4),
                     "old_row_pos": _r(n_old * 8), "top1_idx": _r(B * 4), "top1_d2": _r(B * 4), "top1_xn": _r(B * 4),
                     "top1_labels": _r(B * 4), "partition_cells": _r(K * partition_blocks(n_total, K) * 8)}}
    return MemoryPlan("index-update", n_total, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


INDEX_SCAN_KEYS = 1 << 27        # ops.INDEX_SCAN_KEYS
INDEX_DEEP_OVERSHOOT = 2         # ops.INDEX_DEEP_OVERSHOOT
DEEP_BINS = 256                  # one 8-bit digit


def deep_block_queries(m: int, nprobe: int) -> int:
    """ops.deep_block_queries: queries per block of a deep search."""
    return max(1, 8 * INDEX_SCAN_KEYS // (4 * DEEP_BINS + 28 * int(nprobe) + 8 * INDEX_DEEP_OVERSHOOT * int(m)))


def plan_index_search_deep(n: int, D: int, K: int, dtype="bfloat16", *, nq: int, m: int, nprobe: int) -> MemoryPlan:
    """A deep search (ops.index_search_deep) of ``nq`` queries for ``m`` rows each over ``nprobe``
    lists of an index of ``n`` ids: the index and the result, and per block of queries the two
    phases' scratch -- the radix select's histogram (1 KiB a query), its per-query state and the
    walk's pair arrays; then the range passes' counts and bases and the keys under the radius
    (``INDEX_DEEP_OVERSHOOT * m`` a query where the stop rule holds; rows tied at the m-th place and
    a forced pass count can exceed it) with the sort's copies of them."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    cols = dpad_for(Dp, es) or Dp
    rows = index_tiles(n, K) * 16
    p = {"row_pack": _r(rows * cols * es), "cn": _r(rows * 4), "order": _r(n * 8), "offsets": _r((K + 1) * 8),
         "tile_offsets": _r((K + 1) * 8), "result_keys": _r(nq * m * 8)}
    B = min(int(nq), deep_block_queries(m, nprobe))
    pairs = B * int(nprobe)
    walk = {"queries": _r(B * Dp * es), "query_norms": _r(B * 4), "probes": _r(pairs * 4), "probe_d2": _r(pairs * 4),
            "pair_order": _r(pairs * 8), "pair_offsets": _r((K + 1) * 8), "item_cum": _r((K + 1) * 8),
            "partition_cells": _r(K * partition_blocks(pairs, K) * 8)}
    keys = _r(INDEX_DEEP_OVERSHOOT * m * B * 8)
    tr = {"select": {**walk, "histogram": _r(B * DEEP_BINS * 4), "prefix": _r(B * 4), "rank": _r(B * 8),
                     "hits": _r(B * 8), "candidates": _r(B * 8)},
          "collect": {**walk, "radius": _r(B * 4), "pair_counts": _r(pairs * 8), "pair_base": _r(2 * pairs * 8),
                      "keys": keys, "sorted_keys": keys, "sort_order": keys, "query_ids": keys, "query_order": keys,
                      "block_keys": _r(B * m * 8)}}
    return MemoryPlan("index-search-deep", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


PQ_KSUB = 256                    # ops.PQ_KSUB: codewords of a sub-space
PQ_SCAN_BYTES = 1 << 30          # ops.PQ_SCAN_BYTES
PQ_ENCODE_ROWS = 1 << 18         # ops.PQ_ENCODE_ROWS
PQ_MAX_SPLITS = 8                # csrc/pqplan.h


def pq_block_queries(M: int, m: int, nprobe: int, F: int, splits: int = PQ_MAX_SPLITS) -> int:
    """ops.pq_block_queries: queries per block of a PQ search."""
    return max(1, PQ_SCAN_BYTES // (int(nprobe) * (int(M) * PQ_KSUB * 4 + 8 * int(F) + 16 * int(splits) * int(m))))


def _pq_held(n: int, D: int, K: int, M: int) -> dict:
    """What a PQ index keeps (ops.PQRowIndex.tensors; the codes carry one spare row while they are built)."""
    return {"codes": _r((n + 1) * M), "order": _r(n * 8), "offsets": _r((K + 1) * 8),
            "codebooks": _r(M * PQ_KSUB * (D // M) * 4)}


def plan_pq_index(n: int, D: int, K: int, M: int, dtype="bfloat16", *, block_rows: int | None = None,
                  train_rows: int = 65536) -> MemoryPlan:
    """A product-quantised index of ``n`` rows in ``M`` sub-vectors (ops.pq_build /
    KMeans.build_pq_index): what it keeps -- ``M`` bytes of codes a row, ``order``, ``offsets`` and the
    codebooks -- and the build's scratch: every row's list and position and the partition's cells
    throughout; one block of top-1 output for the lists; the training sample with its gathered rows
    and the sub-space fit's buffers; one pass of residuals (float32 and the rows' dtype), their padded
    sub-vectors, top-1 output and codes for the encoding."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    dsub = D // M
    dsp = padded_cols(dsub, es)
    p = _pq_held(n, D, K, M)
    held = {"labels": _r(n * 4), "row_pos": _r(n * 8), "partition_cells": _r(K * partition_blocks(n, K) * 8)}
    B = min(n, int(block_rows) if block_rows else TOPK_BLOCK_ROWS)
    T = min(n, int(train_rows))
    E = min(n, int(block_rows) if block_rows else PQ_ENCODE_ROWS, PQ_ENCODE_ROWS)
    tr = {"lists": {**held, "top1_idx": _r(B * 4), "top1_d2": _r(B * 4), "top1_xn": _r(B * 4), "top1_labels": _r(B * 4)},
          "train": {**held, "sample_ids": _r(3 * T * 8), "sample_rows": _r(T * Dp * es), "sample_f32": _r(2 * T * D * 4),
                    "residuals": _r(2 * T * D * es), "slice": _r(T * dsp * es), "slice_norms": _r(T * 4),
                    "slice_labels": _r(2 * T * 4), "slice_dist": _r(T * 4),
                    "fit_sums": _r(256 * (PQ_KSUB * dsp + PQ_KSUB) * 8)},
          "encode": {**held, "residual_f32": _r(2 * E * D * 4), "residuals": _r(E * D * es), "slice": _r(E * dsp * es),
                     "top1_idx": _r(E * 4), "top1_d2": _r(E * 4), "top1_xn": _r(E * 4), "codes_block": _r(E * M),
                     "positions": _r(2 * E * 8), "codebook_packs": _r(M * PQ_KSUB * max(dsp, 32) * es * 2)}}
    return MemoryPlan("pq-index", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


def plan_pq_search(n: int, D: int, K: int, M: int, dtype="bfloat16", *, nq: int, m: int, nprobe: int) -> MemoryPlan:
    """A PQ search (ops.pq_search) of ``nq`` queries for ``m`` rows each over ``nprobe`` lists: the index
    and the result, and per block of queries (``pq_block_queries``) the probes, the pairs' residuals
    (float32 and the rows' dtype), one sub-space's padded slice and distances, the tables (``M`` KiB a
    pair) and the keys (``splits * m`` a pair) with the sort's copies."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    dsp = padded_cols(D // M, es)
    p = {**_pq_held(n, D, K, M), "result_keys": _r(nq * m * 8)}
    B = min(int(nq), pq_block_queries(M, m, nprobe, D))
    pairs = B * int(nprobe)
    keys = _r(pairs * PQ_MAX_SPLITS * m * 8)
    tr = {"block": {"queries": _r(B * Dp * es), "query_norms": _r(B * 4), "probes": _r(2 * pairs * 4),
                    "probe_d2": _r(pairs * 4), "probe_centres": _r(pairs * D * 4), "residual_f32": _r(pairs * D * 4),
                    "residuals": _r(pairs * D * es), "slice": _r(pairs * dsp * es), "slice_norms": _r(pairs * 4),
                    "slice_d2": _r(pairs * PQ_KSUB * 4), "tables": _r(pairs * M * PQ_KSUB * 4), "keys": keys,
                    "sorted_keys": keys, "sort_order": keys, "block_keys": _r(B * m * 8)}}
    return MemoryPlan("pq-index-search", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, tr)


def pq_refine_block_queries(M: int, nprobe: int, F: int, shortlist: int, *, host_rows: bool = False,
                            esize: int = 4) -> int:
    """ops.pq_refine_block_queries: queries per block of a refined PQ search."""
    R = int(nprobe) * int(shortlist)
    per = int(nprobe) * (int(M) * PQ_KSUB * 4 + 8 * int(F) + 16 * int(shortlist)) + 32 * R
    if host_rows:
        per += R * (int(F) * int(esize) + 8)
    return max(1, PQ_SCAN_BYTES // per)


def plan_pq_refine(n: int, D: int, K: int, M: int, dtype="bfloat16", *, nq: int, m: int, nprobe: int,
                   shortlist: int = 32, host_rows: bool = False) -> MemoryPlan:
    """A refined PQ search (ops.pq_refine): :func:`plan_pq_search`'s terms with the scan at ``splits = G,
    m = s`` (``G * s = shortlist`` keys a pair, decoded into as many candidate ids), per block of
    queries (``pq_refine_block_queries``) the ``[B, R]`` re-rank keys, ``R = nprobe * shortlist``, with the
    sort's copies and, for rows kept on the host, the staged rows (at most ``B * R``) and the remapped
    ids.  Device rows are the caller's and are read in place."""
    es = esize_of(dtype)
    Dp = padded_cols(D, es)
    dsp = padded_cols(D // M, es)
    S = int(shortlist)
    p = {**_pq_held(n, D, K, M), "result_keys": _r(nq * m * 8)}
    B = min(int(nq), pq_refine_block_queries(M, nprobe, D, S, host_rows=host_rows, esize=es))
    pairs = B * int(nprobe)
    R = int(nprobe) * S
    keys = _r(B * R * 8)
    block = {"queries": _r(B * Dp * es), "query_norms": _r(B * 4), "probes": _r(2 * pairs * 4),
             "probe_d2": _r(pairs * 4), "probe_centres": _r(pairs * D * 4), "residual_f32": _r(pairs * D * 4),
             "residuals": _r(pairs * D * es), "slice": _r(pairs * dsp * es), "slice_norms": _r(pairs * 4),
             "slice_d2": _r(pairs * PQ_KSUB * 4), "tables": _r(pairs * M * PQ_KSUB * 4), "shortlist_keys": keys,
             "candidates": keys, "rerank_keys": keys, "sorted_keys": keys, "sort_order": keys,
             "block_keys": _r(B * m * 8)}
    if host_rows:
        block.update({"staged_rows": _r(min(B * R, n) * D * es), "local_ids": keys, "staged_ids": _r(min(B * R, n) * 8)})
    return MemoryPlan("pq-index-refine", n, D, Dp, K, "bfloat16" if es == 2 else "float32", p, {"block": block})


# ------------------------------------------------------------------------ budget
def hbm_budget(device=None) -> int:
    """Bytes a fit on ``device`` may allocate: ``MIKMEANS_HBM_BYTES`` when set, else the free
    device memory plus the caching allocator's unused reserve, minus headroom (2 % of HBM,
    at least 1 GiB) for the HIP runtime, RCCL buffers and the allocator's own rounding."""
    env = os.environ.get("MIKMEANS_HBM_BYTES")
    if env:
        return int(float(env))
    import torch

    free, total = torch.cuda.mem_get_info(device)
    unused = torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
    return int(free + unused - max(0.02 * total, 1 << 30))


def plan_fit(n: int, D: int, K: int, dtype="bfloat16", *, budget: int, x_on_device: bool,
             weighted: bool = False, incremental: bool = True, init="k-means++",
             n_local_trials: int | None = None, init_rows: int | None = None,
             src_itemsize: int | None = None, empty_policy: str = "keep", copy_x: bool = True,
             max_chunk_rows: int = 1 << 24, bounded: bool = False) -> MemoryPlan:
    """Choose how a Lloyd fit of an ``n``-row shard runs within ``budget`` bytes of HBM:
    resident when it fits (or when X already lives on the device), else streamed in the
    largest power-of-two multiple of 1536 rows that fits; :class:`HBMCapacityError` when
    neither does."""
    res = plan_resident(n, D, K, dtype, weighted=weighted, incremental=incremental, init=init,
                        n_local_trials=n_local_trials, copy_x=copy_x, empty_policy=empty_policy,
                        bounded=bounded, src_itemsize=src_itemsize)
    res.budget = budget
    if res.fits:
        return res
    if x_on_device:
        raise HBMCapacityError(
            f"KMeans.fit: the device-resident shard needs {res.peak / 1e9:.2f} GB of HBM "
            f"({res.summary()}) but only {budget / 1e9:.2f} GB are available; pass the rows as a "
            "host (CPU) tensor to stream them, or use more ranks")
    R = ROW_ALIGN
    while R * 2 <= max_chunk_rows and R < n:
        R *= 2
    while True:
        st = plan_streaming(n, D, K, dtype, chunk_rows=R, weighted=weighted, init=init,
                            n_local_trials=n_local_trials, init_rows=init_rows, src_itemsize=src_itemsize,
                            empty_policy=empty_policy)
        st.budget = budget
        if st.fits:
            return st
        if R <= ROW_ALIGN:
            break
        R //= 2
    raise HBMCapacityError(
        f"KMeans.fit: {n} rows x {D} features need {res.peak / 1e9:.2f} GB resident and "
        f"{st.peak / 1e9:.2f} GB even when streamed in {st.chunk_rows}-row chunks "
        f"(per-row labels and norms stay on the device), but only {budget / 1e9:.2f} GB of HBM "
        "are available; use more ranks (the per-row state divides by the world size)")
