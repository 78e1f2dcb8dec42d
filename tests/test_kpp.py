"""Oracles of the k-means++ seeding kernels (csrc/kpp.hip), checked on the CPU.

tests/test_gpu_kpp.py compares kpp_d2 / kpp_cc / kpp_sample and the whole GPU seeding with the
float64 references built here; this file checks those references themselves wherever the CPU
suite runs: the float64 mirror of the seeding against ``init_kmeanspp`` on CPU tensors, that the
accept set of the real-potential draws decides (almost) every draw, and that the rows built on
the prune boundary really straddle it."""
import functools

import numpy as np
import pytest
import torch

from mikmeans.models.init import init_kmeanspp
from mikmeans.ops import vec_elems
from mikmeans.parallel import Comm

DTYPES = [torch.float32, torch.bfloat16]
U24 = 2.0 ** -24
KPP_PRUNE = 4.004                      # csrc/kpp.hip


def pad_cpu(X: torch.Tensor, dtype) -> torch.Tensor:
    """``X`` stored in ``dtype`` with zero columns up to whole 16-byte pieces (ops.pad_columns on the CPU)."""
    v = vec_elems(dtype)
    n, d = X.shape
    out = torch.zeros((n, (d + v - 1) // v * v), dtype=dtype)
    out[:, :d] = X.to(dtype)
    return out


def d2_bound(width: int, ref: torch.Tensor) -> torch.Tensor:
    """|f32 sum of squared f32 differences - exact| <= this: one rounding for the difference (twice
    in the square), one for the square, fewer than ``width`` for the additions; FMA only lowers it."""
    return 1.01 * (width + 3) * U24 * ref


def block_sums_ref(d2: torch.Tensor, rpb: int) -> np.ndarray:
    """Per-block sums of f32 ``d2`` in extended precision (rounded to f64 at the end)."""
    n = d2.numel()
    nb = max(1, -(-n // rpb))
    buf = np.zeros(nb * rpb, dtype=np.longdouble)
    buf[:n] = d2.double().numpy()
    return buf.reshape(nb, rpb).sum(1).astype(np.float64)


# ----------------------------------------------------------------------------- (g) the mirror
SEED_CASES = [(5000, 24, 40, 1), (5000, 24, 40, 3), (3001, 300, 20, 1), (300_000, 8, 12, 1), (2000, 1024, 16, 3)]
SEED = 5


@functools.lru_cache(maxsize=None)
def seeding_rows(n: int, d: int) -> torch.Tensor:
    """Small-integer rows: exact in bf16, every distance and potential exact in f32 and f64."""
    g = torch.Generator().manual_seed(n + d)
    return torch.randint(-3, 4, (n, d), generator=g).float()


def kpp_mirror(X: torch.Tensor, K: int, seed: int, L: int) -> tuple[list[int], int]:
    """k-means++ / greedy k-means++ in float64 on the same ``default_rng(seed)`` stream as
    models/init.py: (row indices of the K centres, draws that landed exactly on a boundary)."""
    X = X.double()
    n = X.shape[0]
    rng = np.random.default_rng(seed)
    idx = [int(rng.integers(0, n))]
    u = rng.random((K - 1) * L)
    d2 = ((X - X[idx[0]]) ** 2).sum(1)
    on_boundary = 0
    for k in range(1, K):
        cs = torch.cumsum(d2, 0)
        tot = float(cs[-1])
        cand = []
        for t in range(L):
            tv = float(u[(k - 1) * L + t]) * tot
            i = int(torch.searchsorted(cs, torch.tensor([tv], dtype=torch.float64), right=True))
            assert i < n and d2[i] > 0
            on_boundary += tv == float(cs[i] - d2[i])
            cand.append(i)
        pots = [float(torch.minimum(d2, ((X - X[i]) ** 2).sum(1)).sum()) for i in cand]
        best = cand[int(np.argmin(pots))]            # ties -> the first trial
        idx.append(best)
        d2 = torch.minimum(d2, ((X - X[best]) ** 2).sum(1))
    return idx, on_boundary


@functools.lru_cache(maxsize=None)
def mirror_centres(n: int, d: int, K: int, L: int) -> torch.Tensor:
    idx, on_boundary = kpp_mirror(seeding_rows(n, d), K, SEED, L)
    assert on_boundary == 0                          # (no draw depends on how a tie is broken)
    return seeding_rows(n, d)[idx]


# ----------------------------------------------------------------------------- (e), (f) the sampler
def exact_draw(cum: np.ndarray, target: float) -> int:
    """The row kpp_sample must return for integer-valued d2 (``cum``: its exact f64 cumulative sum):
    the first i with d2[i] > 0 and target < cum[i]; past the end the last positive row; an
    all-zero d2 gives row 0; a negative or NaN target gives -1 (not the owner: zeros)."""
    if not target >= 0.0:
        return -1
    total = float(cum[-1])
    if total == 0.0:
        return 0
    if target >= total:
        target = total * (1.0 - 1e-12)
    return int(np.searchsorted(cum, target, side="right"))


def accept_set(cum: np.ndarray, tt: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """Rows [lo, hi] a draw at cumulative potential ``tt`` may return: cum[i-1] - eps <= tt <
    cum[i] + eps with eps = 2 N 2^-53 total, the f64 summation bound on both sides (the kernel
    and the reference associate their sums differently).  lo == hi: the draw is decided."""
    n = cum.shape[0]
    eps = 2.0 * n * 2.0 ** -53 * cum[-1]
    prev = np.concatenate([[0.0], cum[:-1]])
    lo = np.searchsorted(cum + eps, tt, side="right")
    hi = np.searchsorted(prev - eps, tt, side="right") - 1
    return np.minimum(lo, n - 1), np.minimum(hi, n - 1)


@functools.lru_cache(maxsize=None)
def real_potentials(n: int):
    """(d2 f32 [n], u f64 [300], f64 cumulative sum) of test (f)."""
    g = torch.Generator().manual_seed(n)
    d2 = (torch.rand(n, generator=g) ** 4 * 50).float()
    u = torch.rand(300, generator=g, dtype=torch.float64)
    return d2, u, np.cumsum(d2.double().numpy())


# ----------------------------------------------------------------------------- (d) the prune boundary
SWEEP = [0.0] + [sg * 10.0 ** -e for e in range(1, 7) for sg in (1.0, -1.0)]
N_OWNERS = 8


@functools.lru_cache(maxsize=None)
def boundary_rows(d: int, dtype, offset: float) -> torch.Tensor:
    """Rows on the prune boundary, stored in ``dtype`` (CPU, column-padded).  Rows 0..7 are the
    owner centres c_j, row 8 the new centre c.  For every owner, rows on the segment c_j -> c at
    distance R_j / 2.001 (1 + s), s swept through +-{1e-1 .. 1e-6, 0} (16 copies each, jittered by
    a few f32 ulp): cc[owner] >= 4.004 d2 flips at s = 0, and past R_j / 2 the new centre really
    wins.  Plus random rows around every owner (pruned) and around c (not pruned), shuffled."""
    g = torch.Generator().manual_seed(d + int(offset))
    cen = pad_cpu(torch.randn(N_OWNERS + 1, d, generator=g) * 10 + offset, dtype).double()[:, :d]
    c = cen[N_OWNERS]
    rows = []
    for j in range(N_OWNERS):
        R = float((c - cen[j]).norm())
        unit = (c - cen[j]) / R
        for s in SWEEP:
            jit = 1.0 + torch.cat([torch.zeros(1), (torch.rand(15, generator=g) - 0.5) * 4e-7]).double()
            rows.append(cen[j][None, :] + (R / 2.001 * (1.0 + s) * jit)[:, None] * unit[None, :])
        rows.append(cen[j][None, :] + torch.randn(200, d, generator=g).double() * (R / 10 / d ** 0.5))
    R = float((c - cen[0]).norm())
    rows.append(c[None, :] + torch.randn(800, d, generator=g).double() * (R / 10 / d ** 0.5))
    body = torch.cat(rows)
    body = body[torch.randperm(body.shape[0], generator=g)]
    return pad_cpu(torch.cat([cen, body]).float(), dtype)


def prune_shares(X: torch.Tensor) -> tuple[float, float]:
    """(share of rows that meet the prune condition, share that do not) in float64."""
    Xd = X.double()
    cen, c = Xd[:N_OWNERS], Xd[N_OWNERS]
    dist = torch.cdist(Xd, cen) ** 2
    d2, own = dist.min(1)
    cc = ((cen - c) ** 2).sum(1)
    pruned = cc[own] >= KPP_PRUNE * d2
    return float(pruned.double().mean()), float((~pruned).double().mean())


# ----------------------------------------------------------------------------- the CPU tests
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("n,d,K,L", SEED_CASES)
def test_mirror_equals_cpu_seeding(n, d, K, L, dtype):
    """The float64 mirror draws the centres of init_kmeanspp on CPU tensors, row for row."""
    X = seeding_rows(n, d)
    assert torch.equal(X.to(dtype).float(), X)
    C = init_kmeanspp(X.to(dtype), d, K, n, 0, Comm.local("cpu"), seed=SEED, n_local_trials=L)
    assert torch.equal(C, mirror_centres(n, d, K, L))


def test_seeding_rows_have_duplicates():
    """The 300 000-row case draws around zero-potential rows (7^8 distinct rows at most)."""
    X = seeding_rows(300_000, 8)
    assert X.shape[0] - torch.unique(X, dim=0).shape[0] > 5000


@pytest.mark.parametrize("n", [5000, 300_000])
def test_real_potential_draws_are_decided(n):
    """At least 99 % of the draws of test (f) have one acceptable row (the reference alone fixes this)."""
    d2, u, cum = real_potentials(n)
    lo, hi = accept_set(cum, u.numpy() * cum[-1])
    assert bool((lo <= hi).all())
    assert float((lo == hi).mean()) >= 0.99


def test_exact_draw_edges():
    cum = np.cumsum(np.array([0, 0, 3, 0, 2, 0], dtype=np.float64))
    assert [exact_draw(cum, t) for t in (0.0, 2.5, 3.0, 4.5, 5.0, 10.0)] == [2, 2, 4, 4, 4, 4]
    assert exact_draw(cum, -1.0) == -1 and exact_draw(cum, float("nan")) == -1
    assert exact_draw(np.zeros(4), 0.0) == 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("offset", [0.0, 100.0])
@pytest.mark.parametrize("d", [8, 128, 1024])
def test_boundary_rows_straddle_the_prune_condition(d, offset, dtype):
    """The input of test (d) is not vacuous: >= 30 % of its rows are pruned, >= 10 % are not."""
    pruned, kept = prune_shares(boundary_rows(d, dtype, offset))
    assert pruned >= 0.30 and kept >= 0.10, (pruned, kept)
