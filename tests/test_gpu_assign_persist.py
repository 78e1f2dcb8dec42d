"""The persistent assign kernel (csrc/assign16.hip assign16_persist_kernel) against the one-pass
grid, bitwise: labels, distances, inertia / changed-count slot words.  Both kernels run in one
process on the same inputs through the ``assign_persist`` switch (0 = one-pass, 1 = persistent,
n >= 2 = persistent on a grid of n workgroups, so a small N gives every workgroup several row
groups and an uneven last round).  The native binding is called without the centre-split
scratch, so small N takes the one-pass grid too."""
import pytest
import torch

from mikmeans import ops
from mikmeans.ops import pad_columns
from mikmeans.ops.native import slot_totals

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUP = 256   # rows per workgroup / row group at bf16 D=128 (4 waves x 4 blocks x 16)


def _problem(n, k, d=128, seed=0, outlier_rows=()):
    g = torch.Generator().manual_seed(seed + n + k)
    X = torch.randn(n, d, generator=g)
    for row in outlier_rows:
        X[row] *= 300.0
    Xb = pad_columns(X.to(torch.bfloat16).to(DEV))
    C = torch.randn(k, d, generator=g) * 0.8
    pk = ops.pack_centers(C.to(DEV), Xb.shape[1], torch.bfloat16, DEV)
    return Xb, pk, ops.row_sqnorm(Xb)


def _assign(native, Xb, pk, xn, prior=3):
    n = Xb.shape[0]
    lab = torch.full((n,), prior, dtype=torch.int32, device=DEV)
    mind = torch.empty(n, device=DEV)
    slots = torch.zeros(native.NSLOT * native.SLOT_STRIDE, dtype=torch.float64, device=DEV)
    native.assign(Xb, pk.pack, pk.cn, xn, lab, mind, slots, pk.Kpad, pk.dpad, True, None, None, None, None, False,
                  None, None)
    torch.cuda.synchronize()
    return lab, mind, slots.view(torch.int64).clone()


def _compare(native, kvariant, Xb, pk, xn, arms=(5, 1)):
    kvariant("assign_persist", 0)
    ref = _assign(native, Xb, pk, xn)
    for arm in arms:
        kvariant("assign_persist", arm)
        got = _assign(native, Xb, pk, xn)
        assert torch.equal(got[0], ref[0]), f"labels, arm {arm}"
        assert torch.equal(got[1], ref[1]), f"distances, arm {arm}"
        assert torch.equal(got[2], ref[2]), f"slot words, arm {arm}"   # inertia digits + changed count
        assert slot_totals(got[2].view(torch.float64)) == slot_totals(ref[2].view(torch.float64))
    assert slot_totals(ref[2].view(torch.float64))[1] > 0   # (prior labels present: rows did change)
    return ref


@pytest.mark.parametrize("k", [64, 128, 192, 1024])
def test_ring_wrap_and_slot_parity(native, kvariant, k):
    """1, 2, 3 and 16 chunks a pass (64 centres per chunk): with an odd count chunk 0 alternates
    ring slots from pass to pass.  20 row groups and a ragged tail on 5 workgroups."""
    Xb, pk, xn = _problem(5137, k)
    _compare(native, kvariant, Xb, pk, xn)


@pytest.mark.parametrize("n", [100, 10 * GROUP, 3 * GROUP + 17])
def test_row_count_edges(native, kvariant, n):
    """Fewer rows than one group; a whole number of groups; fewer groups than workgroups."""
    Xb, pk, xn = _problem(n, 192)
    _compare(native, kvariant, Xb, pk, xn)


def test_outlier_group_between_ordinary_groups(native, kvariant):
    """A group with an outlier row takes per-point offsets, its neighbours on the same workgroup
    (cap 2: groups 6, 8, 10 ... and 7, 9, ...) the shared offset: both loop copies, the seed
    offset handed from group to group."""
    Xb, pk, xn = _problem(5137, 192, outlier_rows=(8 * GROUP + 10, 13 * GROUP + 255))
    _compare(native, kvariant, Xb, pk, xn, arms=(2, 5, 1))


def test_exact_ties_keep_the_lowest_index(native, kvariant):
    """All-identical rows and duplicated centres: every row takes the lowest of the tied centres."""
    n, k, d = 5137, 128, 128
    g = torch.Generator().manual_seed(5)
    C = torch.randn(k, d, generator=g).to(torch.bfloat16).float()
    C[40] = C[7]
    C[99] = C[7]
    X = C[7].repeat(n, 1)
    Xb = pad_columns(X.to(torch.bfloat16).to(DEV))
    pk = ops.pack_centers(C.to(DEV), Xb.shape[1], torch.bfloat16, DEV)
    xn = ops.row_sqnorm(Xb)
    ref = _compare(native, kvariant, Xb, pk, xn)
    assert bool((ref[0] == 7).all())


def test_repeated_launches_are_identical(native, kvariant):
    """30 launches on 5 workgroups, an outlier group among them, other kernels' LDS and register
    history in between: the same outputs every time."""
    Xb, pk, xn = _problem(5137, 192, outlier_rows=(8 * GROUP + 10,))
    kvariant("assign_persist", 5)
    first = _assign(native, Xb, pk, xn)
    Y = torch.randn(20_000, 256, device=DEV, dtype=torch.bfloat16) * 100
    Cy = torch.randn(512, 256, device=DEV) * 50
    for r in range(30):
        if r % 5 == 4:
            ops.assign(Y, Cy, with_dist=True)
        got = _assign(native, Xb, pk, xn)
        assert all(torch.equal(a, b) for a, b in zip(got, first)), f"launch {r}"


def test_uncapped_grid_over_two_resident_rounds(native, kvariant):
    """The launcher's own grid (occupancy x CUs workgroups): a little over two resident rounds."""
    Xb, pk, xn = _problem(700_001, 1024)
    _compare(native, kvariant, Xb, pk, xn, arms=(1,))


def test_captured_graph_replay_equals_eager(native, kvariant):
    Xb, pk, xn = _problem(40_003, 192, outlier_rows=(4000,))
    kvariant("assign_persist", 0)
    ref = _assign(native, Xb, pk, xn)
    kvariant("assign_persist", 7)
    eager = _assign(native, Xb, pk, xn)   # (also warms the launcher's cached occupancy query)
    n = Xb.shape[0]
    lab = torch.empty(n, dtype=torch.int32, device=DEV)
    mind = torch.empty(n, device=DEV)
    slots = torch.zeros(native.NSLOT * native.SLOT_STRIDE, dtype=torch.float64, device=DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            native.assign(Xb, pk.pack, pk.cn, xn, lab, mind, slots, pk.Kpad, pk.dpad, True, None, None, None, None,
                          False, None, None)
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        lab.fill_(3)
        mind.zero_()
        slots.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got in (eager, (lab, mind, slots.view(torch.int64))):
            assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1]) and torch.equal(got[2], ref[2])
