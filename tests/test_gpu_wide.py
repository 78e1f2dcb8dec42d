"""The wide-row kernels (D 384-1024: csrc/assign16.hip WIDE builds, plain and TOP2; the
K-split and column-slice M-steps of csrc/update.hip at these widths) against float64
references on the host -- always the distances to the QUANTISED centres the kernels rank.

Exact ties and the lowest index, per-point-offset workgroups, the TOP2 bounds within the
score slack the bounded E-step relies on (csrc/rows.hip row_slack), the bounded trajectory
anchored to the f64 argmin, and every M-step plan cell the dispatch reaches above D=256
(routing asserted first, so a plan change cannot quietly move a cell to another kernel)."""
import functools
import math

import pytest
import torch

from mikmeans import ops
from mikmeans.data import blobs as B
from mikmeans.models.lloyd import LloydEngine
from mikmeans.ops import cpu as ref
from mikmeans.parallel import memplan

from .test_gpu_bounded import _spread_rows
from .test_gpu_kernels import _bf16_dist, _check_assign, _first_argmin, _resolvable_argmin

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16

# every wide DPAD for both dtypes, and one ragged width each (300 -> 384, 1000 -> 1024)
WIDE = [(F32, 384), (F32, 512), (F32, 768), (F32, 1024), (F32, 1000),
        (BF16, 384), (BF16, 512), (BF16, 768), (BF16, 1024), (BF16, 300)]


def _id(v):
    if isinstance(v, torch.dtype):
        return "bf16" if v == BF16 else "f32"
    return str(v)


def _setup(X, C):
    """Column-padded device rows, the centre pack and the row norms."""
    Xp = ops.pad_columns(X.to(DEV))
    pk = ops.pack_centers(C.to(DEV), Xp.shape[1], Xp.dtype, DEV)
    assert pk.dpad > 256 and pk.dpad == ops.dpad_for(X.shape[1], X.dtype)
    return Xp, pk, ops.row_sqnorm(Xp)


def _out(native, n):
    return (torch.full((n,), 7, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV),
            torch.zeros(native.NSLOT * native.SLOT_STRIDE, dtype=torch.float64, device=DEV))


def _both_grids(native, Xp, pk, xn):
    """(labels, distances) of the centre-split grid (small batches) after checking that the
    one-pass grid gives the same bits."""
    n = Xp.shape[0]
    assert n <= ops.SPLIT_MAX_ROWS
    ls, ms = ops.assign(Xp, None, with_dist=True, pack=pk)        # centre-split grid
    lo, mo, slots = _out(native, n)
    native.assign(Xp, pk.pack, pk.cn, xn, lo, mo, slots, pk.Kpad, pk.dpad, True, None)   # one pass
    assert torch.equal(ls, lo)
    assert torch.equal(ms, mo)
    return ls.cpu().long(), ms.cpu()


def _f64_dist(X, C):
    """xx, quantised centres and squared distances, f64 on the host."""
    Cq = ref.quantize_centers(C, X.dtype).double()
    Xd = X.double()
    xx = (Xd * Xd).sum(1)
    return xx, Cq, xx[:, None] - 2 * Xd @ Cq.T + (Cq * Cq).sum(1)[None]


# ---- 1. exact ties, lowest index ---------------------------------------------------------
def _tie_problem(d, n=1237, k=1300):
    g = torch.Generator().manual_seed(3 + d)
    X = torch.randint(-2, 2, (n, d), generator=g).float()
    C = torch.randint(-2, 2, (k, d), generator=g).float()
    C[17] = C[5]       # exact duplicate centres: the lower index must win
    C[k - 100] = C[40]
    C[k - 1] = C[300]
    X[:50] = C[5]      # rows sitting exactly on a duplicated centre
    X[50:100] = C[40]
    return X, C


@pytest.mark.parametrize("dtype,d", WIDE, ids=_id)
def test_wide_assign_exact_ties_lowest_index(native, dtype, d):
    """Integer data in [-2, 2): every score is exact in f32 and every bf16 key below 2^15
    (integer gaps of 1 survive the keys' 6 lost mantissa bits), so the labels are the f64
    argmin with the LOWEST index on exact ties, on the centre-split and the one-pass grid.
    K = 1300 crosses the 256-centre key-segment merge and is no multiple of 16."""
    X, C = _tie_problem(d)
    k = C.shape[0]
    xx, _, dist = _f64_dist(X, C)
    # the precondition, checked: keys d^2 + o - |x|^2 with the seed offset o at most
    # (1 + 2^-12) max |x|^2 (csrc/rows.hip seed_offsets; 0 for f32)
    keymax = float((dist + ((1 + 2.0**-12) * xx.max() - xx)[:, None]).max())
    tied = (dist == dist.min(1, keepdim=True).values).sum(1) > 1
    print(f"WIDE-FIG ties {_id(dtype)} D={d}: keymax bound {keymax:.0f}, tied rows {float(tied.float().mean()):.4f}")
    assert keymax < 2**15 and bool(tied.any())
    Xp, pk, xn = _setup(X.to(dtype), C)
    got, mind = _both_grids(native, Xp, pk, xn)
    sc = ref.scores(X.double(), C.double())
    exp = _first_argmin(sc)
    if dtype == F32:
        assert torch.equal(got, exp)
    else:
        # (bf16: the per-point seed offset is added in f32, so two DISTINCT centres with
        # equal exact scores may split by one rounding -- as in the narrow test)
        assert torch.equal(sc.gather(1, got[:, None]), sc.gather(1, exp[:, None]))
        same = (C[got] == C[exp]).all(1)
        assert torch.equal(got[same], exp[same])
        assert torch.equal(got[:100], exp[:100])
    assert int(got.max()) < k
    _check_assign(X.to(dtype), C, got, mind, rel=2e-5 if dtype == F32 else 3e-5)


# ---- 2. per-point-offset workgroups (bf16) -----------------------------------------------
@pytest.mark.parametrize("d", [384, 512, 768, 1024, 300])
def test_wide_assign_bf16_outlier_rows_keep_neighbours_resolved(native, d):
    """Two rows 1e6x their neighbours' |x|^2 switch their workgroups to per-point seed offsets
    (the second instantiation of the wide chunk loop): every other row still resolves at the
    documented key resolution 2^-16 (d1^2 + 3|x|^2) + 2^-20 (|x|^2 + max |c|^2), labels and
    distances, on both grids."""
    n, k = 2011, 300
    g = torch.Generator().manual_seed(7 + d)
    X = torch.randn(n, d, generator=g)
    C = torch.randn(k, d, generator=g)
    X[5] *= 1000.0
    X[n // 2 + 3] *= 1000.0
    Xb = X.to(BF16)
    Xp, pk, xn = _setup(Xb, C)
    got, mind = _both_grids(native, Xp, pk, xn)
    xx, Cq, dist = _bf16_dist(Xb, C)
    exp = _first_argmin(dist)
    srt = dist.sort(1).values
    cmax = (Cq * Cq).sum(1).max()
    tol = 2.0**-16 * (srt[:, 0].clamp_min(0) + 3 * xx) + 2.0**-20 * (xx + cmax)
    ok = (srt[:, 1] - srt[:, 0]) > tol
    print(f"WIDE-FIG outlier bf16 D={d}: resolvable {float(ok.float().mean()):.4f}")
    assert ok.float().mean() > 0.95
    bad = (got != exp) & ok
    assert int(bad.sum()) == 0, f"{int(bad.sum())} wrong labels of {int(ok.sum())} resolvable rows"
    dg = dist.gather(1, got[:, None])[:, 0]
    nb = torch.ones(n, dtype=torch.bool)
    nb[[5, n // 2 + 3]] = False
    err = (mind.double() - dg.clamp_min(0)).abs()
    print(f"WIDE-FIG outlier bf16 D={d}: max err/tol {float((err[nb] / (tol[nb] + 1e-6)).max()):.4f}")
    assert bool((err[nb] <= tol[nb] + 1e-6).all())


# ---- 3. TOP2 bounds within the score slack -----------------------------------------------
def _slack(d2, nterms, cmax, o, xx):
    """csrc/rows.hip row_slack / RowSlack::operator(), in f64: the claimed error of a score."""
    acc = 2.0 * (nterms + 8) * 2.0**-24 * (cmax * cmax + o + 2.0 * xx.sqrt() * cmax)
    return acc + 2.0**-16 * (d2 + (o - xx).abs())


@pytest.mark.parametrize("dtype,d", WIDE, ids=_id)
def test_wide_top2_bounds_within_row_slack(native, dtype, d):
    """The TOP2 build of every wide width: ub^2 / lb^2 are the smallest / second smallest f64
    squared distance within the score slack that licenses skipping rows in the bounded E-step
    (plus 2^-22 d^2 for the f32 sqrt / square round trip), the label's distance is the
    minimum within it, lb >= ub; f32: labels and distances are bitwise the plain one-pass
    kernel's.  Rows with norms spread 1-900x: shared- and per-point-offset workgroups."""
    n, k = 3001, 200
    X = _spread_rows(n, d, d + k, dtype)
    sel = torch.randperm(n, generator=torch.Generator().manual_seed(k))[:k]
    C = X[sel.to(DEV)].float() * 0.7
    Xp, pk, xn = _setup(X, C)
    lab, mind, slots = _out(native, n)
    ub = torch.zeros(n, device=DEV)
    lb = torch.zeros(n, device=DEV)
    pk.assign(Xp, xn, lab, mind, slots, True, ub=ub, lb=lb)
    oseed = pk.seed_offsets(xn)
    o = oseed.cpu().double() if oseed is not None else torch.zeros(n, dtype=torch.float64)
    if dtype == BF16:      # both kinds of workgroup occur: shared offsets and the rows' own
        own = (o - xn.cpu().double() * (1 + 2.0**-12)).abs() <= 2.0**-20 * o
        assert n // 4 < int(own.sum()) < 3 * n // 4, int(own.sum())
    xx, Cq, dist = _f64_dist(X.cpu(), C.cpu())
    dist = dist.clamp_min(0)
    cmax = (Cq * Cq).sum(1).max().sqrt()
    srt = dist.sort(1).values
    d1, d2, d3 = srt[:, 0], srt[:, 1], srt[:, 2]
    sl = functools.partial(_slack, nterms=d, cmax=cmax, o=o, xx=xx)
    rt = 2.0**-22
    got = lab.cpu().long()
    dl = dist.gather(1, got[:, None])[:, 0]
    assert bool((dl - d1 <= sl(dl) + sl(d1)).all())
    ub2, lb2 = ub.cpu().double() ** 2, lb.cpu().double() ** 2
    eu, bu = (ub2 - d1).abs(), sl(d1) + rt * d1
    el, bl = (lb2 - d2).abs(), sl(d2) + rt * d2
    em = (mind.cpu().double() - d1).abs()
    print(f"WIDE-FIG top2 {_id(dtype)} D={d}: max err/slack ub {float((eu / bu).max()):.4f} "
          f"lb {float((el / bl).max()):.4f} mind {float((em / sl(d1)).max()):.4f}")
    assert bool((eu <= bu).all()), float((eu / bu).max())
    assert bool((el <= bl).all()), float((el / bl).max())
    assert bool((em <= sl(d1)).all()), float((em / sl(d1)).max())
    # (the sensitivity check: the THIRD nearest distance in place of the second is outside)
    assert not bool(((lb2 - d3).abs() <= sl(d3) + rt * d3).all())
    assert bool((lb >= ub).all())
    if dtype == F32:
        lo, mo, so = _out(native, n)
        native.assign(Xp, pk.pack, pk.cn, xn, lo, mo, so, pk.Kpad, pk.dpad, True, None)
        assert torch.equal(lo, lab) and torch.equal(mo, mind)


# ---- 4. bounded E-step = full E-step, anchored to f64 ------------------------------------
@pytest.mark.parametrize("dtype,d", WIDE, ids=_id)
def test_wide_bounded_trajectory_bitwise_and_f64(native, dtype, d):
    """10 Lloyd steps with the bounded E-step and with the full one from the same start:
    labels, centres and changed counts bit for bit every step; f32: every step's labels are
    the f64 argmin of the previous centres on the resolvable rows (> 99 % of them); and the
    bounded engine really skips rows."""
    from mikmeans.models.init import init_random
    from mikmeans.parallel import Comm

    n, k = 40_000, 40
    X = B.make_blobs(n, d, k, seed=d, dtype=dtype, device=DEV)
    comm = Comm.local(torch.device(DEV))
    C0 = init_random(X, d, k, n, 0, comm, 3)
    ea = LloydEngine(X, k, comm=comm).set_centers(C0)
    eb = LloydEngine(X, k, comm=comm, bounded=True).set_centers(C0)
    assert eb.bounded and eb.pk.dpad > 256
    Xc = X.cpu() if dtype == F32 else None
    re, fr = [], []
    for it in range(10):
        prev = eb.centers.cpu().clone()
        ea.step()
        eb.step()
        sa, sb = ea.last_stats(), eb.last_stats()
        assert torch.equal(ea.labels, eb.labels), it
        assert torch.equal(ea.centers, eb.centers), it
        assert sa.n_changed == sb.n_changed, it
        assert sb.inertia == pytest.approx(sa.inertia, rel=1e-4), it
        re.append(eb.reassigned)
        if dtype == F32:
            exp, ok = _resolvable_argmin(Xc, prev)
            fr.append(float(ok.float().mean()))
            assert fr[-1] > 0.99, (it, fr)
            assert torch.equal(eb.labels.cpu().long()[ok], exp[ok]), it
    print(f"WIDE-FIG bounded {_id(dtype)} D={d}: reassigned {re} resolvable min {min(fr) if fr else None}")
    assert re[0] == n
    assert min(re) < 0.6 * n, re


# ---- 5. M-step above D=256 ---------------------------------------------------------------
MSTEP_N = 60_007      # ragged; >= 2500 rows in each of up to 24 row chunks (one label: FX_LIM flushes)
# dtype, D, K, K-split plan (lpr, gm) or None, slice width
MSTEP_CELLS = [
    (BF16, 384, 1024, (64, 6), 32), (BF16, 512, 1024, (64, 6), 32),
    (BF16, 384, 4096, (64, 3), 8), (BF16, 512, 4096, (64, 3), 8),
    (BF16, 320, 1024, (64, 6), 32),            # lanes 40-63 of each row group past the row
    (BF16, 512, 300, None, 64), (BF16, 512, 5000, None, 4),
    (BF16, 768, 300, None, 64), (BF16, 768, 2048, None, 16),
    (BF16, 1024, 300, None, 64), (BF16, 1024, 2048, None, 16),
    (F32, 384, 300, None, 64), (F32, 384, 2048, None, 16),
    (F32, 1024, 300, None, 64), (F32, 1024, 2048, None, 16),
    (F32, 256, 5000, (64, 3), 4),
]
LABEL_CASES = ["uniform", "one_label", "sorted", "unassigned"]


def _esize(dtype):
    return 2 if dtype == BF16 else 4


def _ks_gm(ks, lpr):
    """Row groups in flight the plan picks (csrc/plan.h choose_ks)."""
    m = 64.0 / ks
    g = math.ceil((m + 2.5 * math.sqrt(m)) / (64.0 / lpr))
    return 2 if g <= 2 else 3 if g <= 4 else 6


def _assert_route(native, dtype, d, k, ks_plan, sw_exp):
    """The dispatch of csrc/update.hip use_ks / launch_update for a plain full pass."""
    es = _esize(dtype)
    sw = native.update_slice_width(ops.dtype_code(dtype), k, d, False)
    assert sw == sw_exp == memplan.choose_sw(es, k, d, False)[0]
    ks = memplan.choose_ks(es, k, d)
    routed = 0 < sw < d and sw * es < 128 and ks is not None
    assert routed == (ks_plan is not None), (sw, ks)
    if routed:
        assert (ks[2], _ks_gm(ks[0], ks[2])) == ks_plan, ks
    return ks is not None and 0 < sw < d        # both kernels can serve the cell


@functools.lru_cache(maxsize=2)
def _mstep_data(dtype, d, kind):
    """(rows in ``dtype``, the same values f64); the cells of one width run back to back."""
    g = torch.Generator().manual_seed(d * 7 + (kind == "int"))
    if kind == "int":       # integers sit on the fixed-point grid: the sums are exact
        X = torch.randint(-1000, 1000, (MSTEP_N, d), generator=g).float().to(dtype)
    else:
        X = (torch.randn(MSTEP_N, d, generator=g) * 2 + torch.arange(d) * 0.25).to(dtype)
    return X, X.double()


def _labels(case, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    lab = torch.randint(0, k, (n,), generator=g, dtype=torch.int32)
    if case == "one_label":
        lab.fill_(k - 1)
    elif case == "sorted":
        lab = lab.sort().values
    elif case == "unassigned":
        lab[::3] = -1
    return lab


def _f64_sums(Xd, lab, k):
    """f64 index_add_ over the labelled rows (-1 rows into a spare row, dropped)."""
    li = lab.long()
    li = torch.where(li < 0, torch.full_like(li, k), li)
    s = torch.zeros(k + 1, Xd.shape[1], dtype=torch.float64).index_add_(0, li, Xd)
    return s[:k], torch.bincount(li, minlength=k + 1)[:k].double()


def _check_sums(tag, kind, sums, counts, es, ec, colmax):
    """Counts exact; integer data: sums exact; Gaussian data: within count * colmax * 2^-20
    (each contribution rounded once to a grid no coarser than colmax * 2^-20), and a reference
    with two adjacent columns of one label swapped is outside that bound."""
    assert torch.equal(counts.cpu(), ec), tag
    s = sums.cpu()
    if kind == "int":
        assert torch.equal(s, es), tag
        return
    bound = ec[:, None] * colmax[None, :] * 2.0**-20
    err = (s - es).abs()
    m = bound > 0
    print(f"WIDE-FIG mstep {tag}: max err/bound {float((err[m] / bound[m]).max()):.4f}")
    assert bool((err <= bound).all()), tag
    j = int(ec.argmax())
    p = es.shape[1] // 4
    wrong = es.clone()
    wrong[j, 2 * p], wrong[j, 2 * p + 1] = es[j, 2 * p + 1], es[j, 2 * p]
    assert not bool(((s - wrong).abs() <= bound).all()), tag


@pytest.mark.parametrize("case", LABEL_CASES)
@pytest.mark.parametrize("dtype,d,k,ks_plan,sw_exp", MSTEP_CELLS,
                         ids=[f"{_id(c[0])}-{c[1]}-{c[2]}" for c in MSTEP_CELLS])
def test_wide_cluster_sums_vs_f64(native, kvariant, dtype, d, k, ks_plan, sw_exp, case):
    """ops.cluster_sums in every plan cell above D=256 (and the f32 D=256 K-split cell)
    against the f64 index_add_: exact on integer data -- any pair <-> cell or column <-> lane
    mix-up is a hard failure -- and within the fixed-point bound on Gaussian data, bitwise
    repeatable; where both kernels can serve a cell their sums are equal bit for bit."""
    both = _assert_route(native, dtype, d, k, ks_plan, sw_exp)
    lab = _labels(case, MSTEP_N, k, d + k)
    ld = lab.to(DEV)
    for kind in ("int", "gauss"):
        X, Xd = _mstep_data(dtype, d, kind)
        es, ec = _f64_sums(Xd, lab, k)
        colmax = Xd.abs().amax(0)
        Xg = X.to(DEV)
        tag = f"{_id(dtype)} D={d} K={k} {case} {kind}"
        kvariant("update_ks", -1)
        sums, counts = ops.cluster_sums(Xg, ld, k)
        _check_sums(tag, kind, sums, counts, es, ec, colmax)
        again, _ = ops.cluster_sums(Xg, ld, k)          # atomics in another order: same bits
        assert torch.equal(again, sums), tag
        if both:
            for arm in (0, 1):
                kvariant("update_ks", arm)
                s2, c2 = ops.cluster_sums(Xg, ld, k)
                assert torch.equal(s2, sums) and torch.equal(c2, counts), (tag, arm)
            kvariant("update_ks", -1)


@pytest.mark.parametrize("d,k,ksplit", [(384, 1024, True), (768, 300, False)])
def test_wide_gathered_update_vs_f64(native, d, k, ksplit):
    """The gathered M-step passes (mini-batch rows drawn with repeats, native.update(rows=)):
    the K-split kernel staging its rows in LDS at bf16 D=384, the slice kernel at D=768."""
    dt = ops.dtype_code(BF16)
    n, b = MSTEP_N, 30_000
    sw = native.update_slice_width(dt, k, d, False)
    ks = memplan.choose_ks(2, k, d)
    routed = 0 < sw < d and sw * 2 < 128 and ks is not None
    assert routed == ksplit
    if ksplit:    # its staged rows fit beside the cells (csrc/plan.h KS_GLIST_BYTES)
        lds = ks[1] * ks[3] * 8 + ks[1] * 4 + 16 + memplan.KS_LIST_BYTES
        assert lds + 2 * (memplan.KS_NT // 64) * 64 * 8 + 8 <= memplan.UPD_LDS_MAX
    g = torch.Generator().manual_seed(d + k)
    idx = torch.randint(0, n, (b,), generator=g)
    lab = torch.randint(0, k, (b,), generator=g, dtype=torch.int32)
    nch = native.update_n_chunks(dt, k, d, b, False)
    slab = torch.empty(nch * k * d, dtype=torch.int64, device=DEV)
    cnt = torch.empty(nch * k, dtype=torch.int64, device=DEV)
    for kind in ("int", "gauss"):
        X, Xd = _mstep_data(BF16, d, kind)
        Xg = X.to(DEV)
        col_exp, _ = ops.fixed_exps(Xg, None)
        packed = torch.zeros(k * d + k + 2, dtype=torch.float64, device=DEV)
        native.update(Xg, lab.to(DEV), k, slab, cnt, nch, None, col_exp, 0, False, rows=idx.to(DEV))
        native.reduce(slab, cnt, nch, k, d, None, packed, col_exp, 0)
        es, ec = _f64_sums(Xd[idx], lab, k)
        _check_sums(f"gathered bf16 D={d} K={k} {kind}", kind, packed[: k * d].view(k, d),
                    packed[k * d: k * d + k], es, ec, Xd.abs().amax(0))


@pytest.mark.parametrize("dtype,d", [(BF16, 768), (F32, 512)], ids=_id)
def test_wide_incremental_mstep_bitwise_and_f64(native, dtype, d):
    """LloydEngine(incremental=True) at wide D (the delta build of the slice kernel) is the
    full M-step bit for bit over 8 steps with a re-seed; the first step's centres are the f64
    means of its labels within the fixed-point bound / count plus the f32 rounding of a centre."""
    n, K = 60_000, 48
    X = B.make_blobs(n, d, K, seed=3, dtype=dtype, device=DEV)
    C0 = X[:K].float()
    ea = LloydEngine(X, K).set_centers(C0)
    eb = LloydEngine(X, K, incremental=True).set_centers(C0)
    assert eb.delta is not None
    KD = K * ea.Dp
    for it in range(8):
        if it == 5:  # re-seed: most labels change -> list overflow / full pass
            C1 = X[K: 2 * K].float()
            ea.set_centers(C1)
            eb.set_centers(C1)
        ea.step()
        eb.step()
        torch.cuda.synchronize()
        assert torch.equal(ea.packed[: KD + K], eb.packed[: KD + K]), it
        assert torch.equal(ea.centers, eb.centers), it
        sa, sb = ea.last_stats(), eb.last_stats()
        assert sa.n_changed == sb.n_changed and sa.inertia == sb.inertia
        if it == 0:
            Xd = X.cpu().double()
            es, ec = _f64_sums(Xd, eb.labels.cpu(), K)
            m = ec > 0
            exp = es[m] / ec[m][:, None]
            tol = Xd.abs().amax(0)[None, :] * 2.0**-20 + 2.0**-24 * exp.abs()
            err = (eb.centers.cpu().double()[m] - exp).abs()
            print(f"WIDE-FIG incremental {_id(dtype)} D={d}: max err/tol {float((err / tol).max()):.4f}")
            assert int(m.sum()) > K // 2 and bool((err <= tol).all())
