"""The k-means++ seeding kernels (csrc/kpp.hip: kpp_d2, kpp_cc, kpp_sample) against float64
references of their own operations, through the bindings models/init.py calls (1 GPU).

References are computed on the CPU in float64 from the stored values (the bf16-rounded rows, the
f32 centre); the oracles shared with the CPU suite live in tests/test_kpp.py, which checks them
there.  Shapes are the smallest that reach each path of the kernels: every lanes-per-row arm,
ragged last column passes, strided rows, block sizes off the kernel's period, more than 1024
blocks, more than 1024 rows per block, zero-potential blocks, the three sampler modes, and both
forms of the pruned pass' centre-centre gather."""
import functools

import numpy as np
import pytest
import torch

from mikmeans import ops
from mikmeans.models.init import _local_target, init_kmeanspp
from mikmeans.parallel import Comm

from . import test_kpp as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = O.DTYPES
IDS = ["f32", "bf16"]


def _nb(n, rpb):
    return max(1, -(-n // rpb))


def _d2_pass(native, X, c, first, d2, rpb, owner=None, cc=None, kcc=0, knew=-1):
    """One kpp_d2 launch; returns its block sums (NaN beforehand: every entry must be written)."""
    bs = torch.full((_nb(X.shape[0], rpb),), float("nan"), dtype=torch.float64, device=DEV)
    if owner is None:
        native.kpp_d2(X, c, first, d2, bs, rpb)
    else:
        native.kpp_d2(X, c, first, d2, bs, rpb, owner, cc, kcc, knew)
    return bs


def _first_pass(native, X, c, rpb):
    d2 = torch.full((X.shape[0],), float("nan"), dtype=torch.float32, device=DEV)
    return d2, _d2_pass(native, X, c, True, d2, rpb)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _check_block_sums(d2, bs, rpb, exact):
    ref = O.block_sums_ref(d2.cpu(), rpb)
    got = bs.cpu().numpy()
    if exact:
        assert np.array_equal(got, ref)
    else:
        assert bool((np.abs(got - ref) <= rpb * 2.0 ** -53 * np.abs(ref)).all())


# ----------------------------------------------------------------------------- (a) kpp_d2
PAIRS = [(1, 256), (255, 256), (257, 256), (5000, 256), (5000, 1000), (4099, 4099), (70001, 35)]
WIDTHS = {torch.float32: [4, 8, 16, 20, 32, 64, 68, 300, 1024],
          torch.bfloat16: [8, 16, 32, 40, 64, 128, 136, 600, 1024]}
# (N, rows_per_block) pairs of the i-th width: every width meets >= 2 pairs, every pair >= 3 widths
WIDTH_PAIRS = [(0, 3, 6), (1, 6), (2, 6), (0, 3, 5), (1, 4), (2, 5), (3, 4, 6), (1, 3, 4), (0, 2, 5)]
assert all(sum(p in wp for wp in WIDTH_PAIRS) >= 3 for p in range(len(PAIRS)))
D2_CASES = [pytest.param(dt, w, WIDTH_PAIRS[i], id=f"{IDS[DTYPES.index(dt)]}-{w}")
            for dt in DTYPES for i, w in enumerate(WIDTHS[dt])]


def _check_d2(native, X, rpb, exact):
    """First pass against float64, second pass == bitwise minimum, block sums after each."""
    n, w = X.shape
    Xg, Xd = X.to(DEV), X.double()
    refs, outs = [], []
    for i in (n // 3, n - 1):                          # centres: data rows
        c = X[i].float()
        refs.append(((Xd - c.double()[None, :]) ** 2).sum(1))
        outs.append(_first_pass(native, Xg, c.to(DEV), rpb))
    d2m = outs[0][0].clone()
    bsm = _d2_pass(native, Xg, X[n - 1].float().to(DEV), False, d2m, rpb)
    ratio = 0.0
    for ref, (d2, bs) in zip(refs, outs):
        got = d2.cpu().double()
        err, bound = (got - ref).abs(), O.d2_bound(w, ref)
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())   # (NaN fails)
        if exact:
            assert torch.equal(got, ref)
        ratio = max(ratio, float((err / bound.clamp_min(1e-300)).max()))
        _check_block_sums(d2, bs, rpb, exact)
    assert torch.equal(_bits(d2m), _bits(torch.minimum(outs[0][0], outs[1][0])))
    _check_block_sums(d2m, bsm, rpb, exact)
    return ratio


@pytest.mark.parametrize("dtype,w,pairs", D2_CASES)
def test_kpp_d2_matches_float64(native, dtype, w, pairs):
    """Every d2[i] within 1.01 (D + 3) 2^-24 of the float64 distance (derived, see d2_bound), the
    second pass the bitwise minimum of two first passes, every block sum the sum of the returned
    d2 within the f64 summation bound -- exactly so on small-integer rows."""
    worst = 0.0
    for p in pairs:
        n, rpb = PAIRS[p]
        g = torch.Generator().manual_seed(1000 * w + n)
        for offset in (0.0, 40.0):
            X = O.pad_cpu(torch.randn(n, w, generator=g) * 3 + offset, dtype)
            worst = max(worst, _check_d2(native, X, rpb, exact=False))
        _check_d2(native, O.pad_cpu(torch.randint(-3, 4, (n, w), generator=g).float(), dtype), rpb, exact=True)
    print(f"kpp_d2 {IDS[DTYPES.index(dtype)]} D={w}: largest error/bound = {worst:.4f}")


def test_kpp_d2_refuses_rows_wider_than_lds(native):
    X = torch.zeros((2, 16380), dtype=torch.float32, device=DEV)
    with pytest.raises(RuntimeError, match="at most 16376 columns"):
        native.kpp_d2(X, torch.zeros(16380, device=DEV), True, torch.zeros(2, device=DEV),
                      torch.zeros(1, dtype=torch.float64, device=DEV), 256)


# ----------------------------------------------------------------------------- (b) strided rows
@pytest.mark.parametrize("dtype,w", [(torch.float32, 8), (torch.float32, 300), (torch.bfloat16, 16),
                                     (torch.bfloat16, 600)])
def test_strided_rows_equal_contiguous(native, dtype, w):
    """X = W[:, :D] of a wider tensor (row stride > D): d2, block sums and the drawn row are
    bitwise those of the contiguous copy."""
    n, rpb = 5000, 256
    g = torch.Generator().manual_seed(w)
    W = (torch.randn(n, w + 24, generator=g) * 3 + 5).to(dtype).to(DEV)
    Xs, Xc = W[:, :w], W[:, :w].contiguous()
    assert Xs.stride(0) > w and not Xs.is_contiguous()
    c1, c2 = Xc[11].float(), Xc[n - 2].float()
    u = torch.tensor([0.37], dtype=torch.float64, device=DEV)
    res = []
    for X in (Xs, Xc):
        d2, bs1 = _first_pass(native, X, c1, rpb)
        first = d2.clone()
        bs2 = _d2_pass(native, X, c2, False, d2, rpb)
        row = torch.full((w,), 7.0, device=DEV)
        idx = torch.full((1,), -9, dtype=torch.int64, device=DEV)
        native.kpp_sample(bs2, d2, rpb, u, X, row, idx, 1, None, 0)
        res.append((first, bs1, d2, bs2, row, idx))
    for a, b in zip(*res):
        assert torch.equal(_bits(a), _bits(b))
    assert torch.equal(res[0][4], Xc[int(res[0][5])].float())


# ----------------------------------------------------------------------------- (c) kpp_cc
@pytest.mark.parametrize("k,d", [(0, 8), (1, 4), (3, 20), (4, 64), (5, 65), (130, 300), (1000, 1024)])
def test_kpp_cc_matches_float64(native, k, d):
    """cc[j] = |cnew - C[j]|^2 within the derived bound for the k chosen centres of a larger
    centres tensor; cc past k stays untouched."""
    g = torch.Generator().manual_seed(k + d)
    worst = 0.0
    for offset in (0.0, 40.0):
        C = torch.randn(k + 3, d, generator=g) * 3 + offset
        cnew = C[k + 1].clone() if k != 3 else C[1].clone()          # (k = 3: one distance is 0)
        cc = torch.full((k + 3,), -7.0, device=DEV)
        native.kpp_cc(C.to(DEV), k, cnew.to(DEV), cc)
        got = cc.cpu().double()
        ref = ((C[:k].double() - cnew.double()[None, :]) ** 2).sum(1)
        err, bound = (got[:k] - ref).abs(), O.d2_bound(d, ref)
        assert bool((err <= bound).all())
        assert bool((got[k:] == -7.0).all())
        if k:
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"kpp_cc k={k} D={d}: largest error/bound = {worst:.4f}")


# ----------------------------------------------------------------------------- (d) pruning
def _check_pruned(native, X, c, d2_0, owner0, cc, k, rpb):
    """From the same state, a pruned and an unpruned pass give bitwise equal d2 and block sums;
    owner becomes k exactly where the d2 bits changed (knew = k), or stays (knew = -1)."""
    d2_u = d2_0.clone()
    bs_u = _d2_pass(native, X, c, False, d2_u, rpb)
    changed = _bits(d2_u) != _bits(d2_0)
    for knew in (k, -1):
        d2_p, own = d2_0.clone(), owner0.clone()
        bs_p = _d2_pass(native, X, c, False, d2_p, rpb, own, cc, k, knew)
        assert torch.equal(_bits(d2_p), _bits(d2_u))
        assert torch.equal(_bits(bs_p), _bits(bs_u))
        exp = torch.where(changed, torch.full_like(owner0, k), owner0) if knew >= 0 else owner0
        assert torch.equal(own, exp)
    return changed


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("d", [8, 128, 1024])
def test_pruned_equals_unpruned_on_the_boundary(native, d, offset, dtype):
    """Rows built on the prune boundary (test_kpp.boundary_rows): rows 0..7 own every d2, row 8 is
    the new centre.  d2 / owner are the minimum / first argmin of eight first passes."""
    X = O.boundary_rows(d, dtype, offset).to(DEV)
    n, w = X.shape
    k, rpb = O.N_OWNERS, 256
    C = torch.zeros((k + 4, w), dtype=torch.float32, device=DEV)
    C[:k + 1] = X[:k + 1].float()
    alone = torch.stack([_first_pass(native, X, C[j], rpb)[0] for j in range(k)])
    d2_0 = alone.min(0).values
    owner0 = (alone == d2_0[None, :]).int().argmax(0).int()           # (ties: the first centre)
    cc = torch.full((k + 4,), float("nan"), device=DEV)
    native.kpp_cc(C, k, C[k], cc)
    pruned = cc[owner0.long()] >= torch.tensor(O.KPP_PRUNE, dtype=torch.float32) * d2_0     # the kernel's own test
    assert 0.30 <= float(pruned.float().mean()) <= 0.90
    changed = _check_pruned(native, X, C[k], d2_0, owner0, cc, k, rpb)
    assert not bool((changed & pruned).any())
    assert 0.05 * n < int(changed.sum()) < n


@functools.lru_cache(maxsize=None)
def _fabricated_history(kcc, dtype):
    """5000 rows of width 8 (half of them near the new centre, row 7), kcc random centres and
    each row's float64-nearest centre with its distance rounded to f32."""
    n, d = 5000, 8
    g = torch.Generator().manual_seed(kcc)
    C = torch.randn(kcc, d, generator=g) * 3
    X = torch.randn(n, d, generator=g) * 3
    X[n // 2:] = X[7][None, :] + torch.randn(n - n // 2, d, generator=g) * 0.05
    X = O.pad_cpu(X, dtype)
    d2, owner = [], []
    for r0 in range(0, n, 500):
        v, i = (torch.cdist(X[r0:r0 + 500].double(), C.double()) ** 2).min(1)
        d2.append(v.float())
        owner.append(i.int())
    return X, C, torch.cat(d2), torch.cat(owner)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("kcc", [16384 - 16, 16384 - 8, 16384, 16385, 20000])
def test_pruned_equals_unpruned_many_centres(native, kcc, dtype):
    """A fabricated history of kcc centres around the LDS size rule at D = 8 (centre + distances +
    the reduction buffer within 64 KiB up to kcc = 16368; the global-memory gather past it)."""
    X, C, d2_0, owner0 = (t.to(DEV) for t in _fabricated_history(kcc, dtype))
    cc = torch.full((kcc + 1,), float("nan"), device=DEV)
    cnew = X[7].float()
    native.kpp_cc(C, kcc, cnew, cc)
    ref = ((C.double() - cnew.double()[None, :]) ** 2).sum(1)
    assert bool(((cc[:kcc].double() - ref).abs() <= O.d2_bound(8, ref)).all())
    changed = _check_pruned(native, X, cnew, d2_0, owner0, cc, kcc, 256)
    n = X.shape[0]
    assert int(owner0.min()) < 100 and int(owner0.max()) >= kcc - 100             # both ends of the gather
    assert 0.3 * n < int(changed.sum()) < 0.7 * n


# ----------------------------------------------------------------------------- (e) kpp_sample, exact
def _int_rows(n, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return O.pad_cpu(torch.randint(-50, 51, (n, 8), generator=g).float(), dtype)


def _int_potential(n, rpb, seed):
    """Small non-negative integers, more than half of them 0: leading and trailing runs of zeros
    and whole zero blocks in the middle."""
    g = torch.Generator().manual_seed(seed)
    d2 = torch.randint(1, 6, (n,), generator=g).float()
    d2[torch.rand(n, generator=g) < 0.5] = 0.0
    nb = _nb(n, rpb)
    if n > 1:
        d2[: min(n // 5, 300)] = 0.0
        d2[n - min(n // 7, 200):] = 0.0
    for b in ({1, nb // 2, nb // 2 + 1} if nb >= 4 else ()):
        d2[b * rpb:(b + 1) * rpb] = 0.0
    if n == 1:
        d2[0] = 3.0
    return d2


def _draws(native, bs, d2, rpb, tg, X, mode, totals=None, rank=0):
    """One launch per target, each on a one-element slice; one host read at the end."""
    T = tg.numel()
    rows = torch.full((T, X.shape[1]), 7.0, device=DEV)
    idx = torch.full((T,), -9, dtype=torch.int64, device=DEV)
    tg = tg.to(DEV)
    for t in range(T):
        native.kpp_sample(bs, d2, rpb, tg[t:t + 1], X, rows[t], idx[t:t + 1], mode, totals, rank)
    return rows.cpu(), idx.cpu()


def _check_draws(rows, idx, exp, X, d2):
    exp = torch.as_tensor(np.asarray(exp), dtype=torch.int64)
    assert torch.equal(idx, exp), (idx[idx != exp][:5], exp[idx != exp][:5])
    want = X.float()[exp.clamp_min(0)] * (exp >= 0).float()[:, None]
    assert torch.equal(_bits(rows), _bits(want + 0.0))               # (not the owner: +0.0 rows)
    if float(d2.sum()) > 0:
        assert bool((d2[exp[exp >= 0]] > 0).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,rpb", [(1, 256), (700, 256), (5000, 256), (5000, 3000), (300_000, 256), (9001, 9001)])
def test_kpp_sample_exact_potentials(native, n, rpb, dtype):
    """Integer potentials: every partial sum is exact in any order, so the drawn row is the first
    i with d2[i] > 0 and target < cum[i], with no tolerance -- at every block boundary (+-0.5), 0,
    the total and past it, random half-integers, in the three modes."""
    X = _int_rows(n, dtype, n + rpb)
    d2 = _int_potential(n, rpb, n + rpb + 1)
    cum = np.cumsum(d2.double().numpy())
    total = float(cum[-1])
    assert total > 0 and float((d2 == 0).float().mean()) >= 0.5 or n == 1
    ends = cum[np.minimum(np.arange(1, _nb(n, rpb) + 1) * rpb, n) - 1]
    rng = np.random.default_rng(n)
    half = rng.integers(0, int(total), 200) + 0.5
    # whole numbers too: most equal a cum[i] inside a block, where `<` and `<=` part in stage 2
    half = np.concatenate([half, rng.integers(0, int(total), 200).astype(np.float64)])
    Xg, d2g = X.to(DEV), d2.to(DEV)
    bs = torch.as_tensor(O.block_sums_ref(d2, rpb), device=DEV)
    # mode 0: the target itself
    tg = np.concatenate([ends, ends - 0.5, ends + 0.5, [0.0, total - 0.5, total, 2 * total], half,
                         [-3.0, float("nan")]])
    rows, idx = _draws(native, bs, d2g, rpb, torch.as_tensor(tg), Xg, 0)
    _check_draws(rows, idx, [O.exact_draw(cum, float(t)) for t in tg], X, d2)
    # mode 1: u, scaled by the kernel's own total (exact); the reference scales it the same way
    sub = ends[:: max(1, len(ends) // 50)]
    u = np.concatenate([sub, sub - 0.5, [0.0, total - 0.5, total], half])
    u = u[u >= 0] / total
    rows, idx = _draws(native, bs, d2g, rpb, torch.as_tensor(u), Xg, 1)
    _check_draws(rows, idx, [O.exact_draw(cum, float(t)) for t in u * total], X, d2)
    # mode 2: four ranks hold this d2; ranks 1 and 3 carry its potential, 0 and 2 none
    if n not in (5000, 9001):
        return
    totals = torch.tensor([0.0, total, 0.0, total], dtype=torch.float64)
    u = np.concatenate([half[:60] / (2 * total), (half[:60] + total) / (2 * total),
                        [0.0, 0.5, (total - 0.5) / (2 * total), 1.0, 1.5]])
    owners = torch.zeros(len(u), dtype=torch.int64)
    for rank in range(4):
        exp = [O.exact_draw(cum, float(_local_target(totals, torch.tensor(v, dtype=torch.float64), rank)[0]))
               for v in u]
        rows, idx = _draws(native, bs, d2g, rpb, torch.as_tensor(u), Xg, 2, totals.to(DEV), rank)
        _check_draws(rows, idx, exp, X, d2)
        owners += idx >= 0
        if rank in (0, 2):
            assert bool((idx == -1).all())
    assert bool((owners == 1).all())                                  # exactly one rank returns a row


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_kpp_sample_all_zero_potential(native, dtype):
    n, rpb = 5000, 256
    X = _int_rows(n, dtype, 3)
    d2 = torch.zeros(n)
    bs = torch.zeros(_nb(n, rpb), dtype=torch.float64, device=DEV)
    tg = torch.tensor([0.0, 0.5, 7.0], dtype=torch.float64)
    for mode in (0, 1):
        rows, idx = _draws(native, bs, d2.to(DEV), rpb, tg, X.to(DEV), mode)
        _check_draws(rows, idx, [0, 0, 0], X, d2)


# ----------------------------------------------------------------------------- (f) kpp_sample, real
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n", [5000, 300_000])
def test_kpp_sample_real_potentials(native, n, dtype):
    """d2 = rand^4 50, mode 1, 300 draws against the float64 cumulative sum: every decided draw
    (one row in the accept set; >= 99 % are, tests/test_kpp.py) is exactly that row, the others
    fall inside the set, none has d2 == 0.  The block sums are float64 sums per block taken on
    the CPU (not kpp_d2's own order; the accept set covers either association)."""
    rpb = 256
    d2, u, cum = O.real_potentials(n)
    X = _int_rows(n, dtype, n)
    bs = torch.as_tensor(O.block_sums_ref(d2, rpb), device=DEV)
    rows, idx = _draws(native, bs, d2.to(DEV), rpb, u, X.to(DEV), 1)
    lo, hi = (torch.as_tensor(a) for a in O.accept_set(cum, u.numpy() * cum[-1]))
    assert float((lo == hi).double().mean()) >= 0.99
    assert bool(((idx >= lo) & (idx <= hi)).all())
    assert bool((d2[idx] > 0).all())
    assert torch.equal(_bits(rows), _bits(X.float()[idx]))


# ----------------------------------------------------------------------------- (g) the whole seeding
@functools.lru_cache(maxsize=None)
def _cpu_centres(n, d, K, L, dtype):
    return init_kmeanspp(O.seeding_rows(n, d).to(dtype), d, K, n, 0, Comm.local("cpu"), seed=O.SEED,
                         n_local_trials=L)


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "unpruned"])
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,d,K,L", O.SEED_CASES)
def test_seeding_equals_float64_mirror(native, n, d, K, L, dtype, prune):
    """On small-integer rows every distance and potential is exact in the kernels and in float64:
    init_kmeanspp on the GPU returns the centres of the independent float64 mirror and of the CPU
    path, row for row, with no tolerance."""
    X = ops.pad_columns(O.seeding_rows(n, d).to(DEV), dtype)
    C = init_kmeanspp(X, d, K, n, 0, Comm.local(DEV), seed=O.SEED, n_local_trials=L, prune=prune).cpu()
    assert torch.equal(C, O.mirror_centres(n, d, K, L))
    assert torch.equal(C, _cpu_centres(n, d, K, L, dtype))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("n,d,K,L", [O.SEED_CASES[0], O.SEED_CASES[1]])
def test_seeding_owner_path_equals_float64_mirror(native, n, d, K, L, dtype):
    """The multi-rank owner path on one rank without a process group (sampler mode 2 end to end)."""
    X = ops.pad_columns(O.seeding_rows(n, d).to(DEV), dtype)
    C = init_kmeanspp(X, d, K, n, 0, Comm.local(DEV), seed=O.SEED, n_local_trials=L, owner_path=True).cpu()
    assert torch.equal(C, O.mirror_centres(n, d, K, L))
