"""The assign's per-group seed statistics (csrc/finalize.hip group_norm_stats, ops/cpu.py
group_norm_stats): (max, min) of the row norms over each 256-row group, the last group over its
valid rows -- the two numbers a bf16 assign workgroup decides its seed offsets from
(csrc/assign16.hip: per-point offsets where max > 4 min).  CPU reference against
``xn.view(-1, 256).amax / .amin``."""
import pytest
import torch

from mikmeans.ops import cpu

GROUP = 256


def _norms(n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    xn = torch.rand(n, generator=g) * 0.5 + 100.0     # within a factor 4 of each other: shared offsets
    return xn


def _reference(xn):
    """amax / amin over whole groups; the ragged tail padded with its last valid row (a clamped lane
    repeats it, which changes neither extreme)."""
    n = xn.numel()
    pad = (-n) % GROUP
    v = torch.cat([xn, xn[-1:].expand(pad)]) if pad else xn
    v = v.view(-1, GROUP)
    return torch.stack([v.amax(1), v.amin(1)], 1)


@pytest.mark.parametrize("n", [256, 257, 5 * 256 + 37])
def test_table_equals_amax_amin_per_group(n):
    xn = _norms(n)
    got = cpu.group_norm_stats(xn)
    assert got.dtype == torch.float32 and got.shape == (-(-n // GROUP), 2)
    assert torch.equal(got, _reference(xn))
    assert not bool((got[:, 0] > 4.0 * got[:, 1]).any())


@pytest.mark.parametrize("n", [256, 257, 5 * 256 + 37])
def test_zero_and_huge_norm_in_one_group_flip_the_decision(n):
    """A row of norm 0 and a row 10^6 times larger than the rest in the first group: that group alone
    takes per-point offsets."""
    xn = _norms(n, seed=1)
    xn[3] = 0.0
    xn[200] = 1.0e8
    got = cpu.group_norm_stats(xn)
    assert torch.equal(got, _reference(xn))
    ppo = got[:, 0] > 4.0 * got[:, 1]
    assert bool(ppo[0]) and int(ppo.sum()) == 1
    assert got[0].tolist() == [1.0e8, 0.0]


def test_ragged_tail_covers_only_its_valid_rows():
    xn = _norms(2 * GROUP + 3, seed=2)
    xn[2 * GROUP:] = torch.tensor([7.0, 5.0, 6.0])
    got = cpu.group_norm_stats(xn)
    assert got[2].tolist() == [7.0, 5.0]
