"""The assign's per-group seed statistics on the GPU (bf16 D=128 K=1024): the table kernel
(csrc/finalize.hip group_norm_stats) against the CPU reference, and both assign kernels reading
their seed decision from it (AssignArgs::gstats) against the same kernels reducing the norms
themselves -- labels, distances and the raw inertia / changed-count slot words, bitwise.  The
persistent kernel is forced through the ``assign_persist`` switch as in
tests/test_gpu_assign_persist.py (5 workgroups over 20 row groups and a ragged tail); the native
binding is called without the centre-split scratch, so small N takes the one-pass grid."""
import pytest
import torch

from mikmeans import ops
from mikmeans.ops import cpu, pad_columns
from mikmeans.ops.native import slot_totals

pytestmark = pytest.mark.gpu
DEV = "cuda"
GROUP = 256
D, K = 128, 1024
N_PERSIST = 20 * GROUP + 17
N_ONEPASS = 3 * GROUP + 5
INPUTS = ["blobs", "outlier", "equal"]


def _rows(kind, n, seed=0):
    g = torch.Generator().manual_seed(seed + n)
    C = torch.randn(K, D, generator=g) * 0.8
    if kind == "equal":      # every row the same: exact ties in every group
        X = C[7].repeat(n, 1)
    else:                    # blobs round the centres, far enough from the origin for shared offsets
        X = C[torch.randint(0, K, (n,), generator=g)] + 3.0 + 0.1 * torch.randn(n, D, generator=g)
        if kind == "outlier":
            X[min(n - 1, 8 * GROUP + 10)] *= 300.0
    return X, C


@pytest.fixture(scope="module")
def problems():
    """(rows, pack, norms, table) per (input, N), built once and left unchanged."""
    out = {}
    for kind in INPUTS:
        for n in (N_PERSIST, N_ONEPASS):
            X, C = _rows(kind, n)
            Xb = pad_columns(X.to(torch.bfloat16).to(DEV))
            pk = ops.pack_centers(C.to(DEV), Xb.shape[1], torch.bfloat16, DEV)
            xn = ops.row_sqnorm(Xb)
            out[kind, n] = (Xb, pk, xn, pk.group_stats(xn))
    return out


def _assign(native, Xb, pk, xn, gstats, prior=3):
    n = Xb.shape[0]
    lab = torch.full((n,), prior, dtype=torch.int32, device=DEV)
    mind = torch.empty(n, device=DEV)
    slots = torch.zeros(native.NSLOT * native.SLOT_STRIDE, dtype=torch.float64, device=DEV)
    native.assign(Xb, pk.pack, pk.cn, xn, lab, mind, slots, pk.Kpad, pk.dpad, True, gstats=gstats)
    torch.cuda.synchronize()
    return lab, mind, slots.view(torch.int64).clone()


def _same(got, ref, what):
    assert torch.equal(got[0], ref[0]), f"labels, {what}"
    assert torch.equal(got[1], ref[1]), f"distances, {what}"
    assert torch.equal(got[2], ref[2]), f"slot words, {what}"


def _table_reference(xn):
    return cpu.group_norm_stats(xn.cpu())


@pytest.mark.parametrize("n", [5 * GROUP + 37, 1536 * 3])
def test_table_kernel_equals_the_cpu_reference(native, n):
    g = torch.Generator().manual_seed(n)
    xn = torch.rand(n, generator=g) * 0.5 + 100.0
    xn[GROUP + 3] = 0.0          # a zero norm and one 10^6 times the rest, in one group
    xn[GROUP + 200] = 1.0e8
    got = torch.empty((-(-n // GROUP), 2), dtype=torch.float32, device=DEV)
    native.group_norm_stats(xn.to(DEV), got, 0)
    ref = _table_reference(xn)
    assert torch.equal(got.cpu(), ref)
    assert int((ref[:, 0] > 4.0 * ref[:, 1]).sum()) == 1
    with pytest.raises(RuntimeError):
        native.group_norm_stats(xn.to(DEV), got, 100)   # (not on the group grid)


@pytest.mark.parametrize("kind", INPUTS)
def test_persistent_kernel_with_the_table(native, kvariant, problems, kind):
    Xb, pk, xn, gs = problems[kind, N_PERSIST]
    assert gs is not None and torch.equal(gs.cpu(), _table_reference(xn))
    ppo = gs[:, 0] > 4.0 * gs[:, 1]
    # one outlier row: exactly its group takes per-point offsets, its neighbours the shared one
    assert int(ppo.sum()) == (1 if kind == "outlier" else 0)
    if kind == "outlier":
        assert bool(ppo[8]) and not bool(ppo[7]) and not bool(ppo[9])
    kvariant("assign_persist", 0)
    onepass = _assign(native, Xb, pk, xn, None)
    kvariant("assign_persist", 5)
    plain = _assign(native, Xb, pk, xn, None)
    table = _assign(native, Xb, pk, xn, gs)
    _same(table, plain, "persistent: table against its own reduction")
    _same(table, onepass, "persistent with the table against the one-pass kernel")
    assert slot_totals(onepass[2].view(torch.float64))[1] > 0   # (prior labels present: rows did change)
    if kind == "equal":
        assert bool((table[0] == 7).all())


@pytest.mark.parametrize("kind", INPUTS)
def test_one_pass_kernel_with_the_table(native, kvariant, problems, kind):
    Xb, pk, xn, gs = problems[kind, N_ONEPASS]
    kvariant("assign_persist", 0)
    plain = _assign(native, Xb, pk, xn, None)
    table = _assign(native, Xb, pk, xn, gs)
    _same(table, plain, "one-pass: table against its own reduction")
    assert slot_totals(plain[2].view(torch.float64))[1] > 0


@pytest.mark.parametrize("persist", [0, 1])
def test_two_lloyd_steps_with_and_without_the_table(native, kvariant, persist):
    """LloydEngine over more rows than the centre split takes (so the plain pass runs), an outlier row
    among them: centres, counts, labels and inertia after two steps."""
    from mikmeans.models.lloyd import LloydEngine

    n = (1 << 18) + 1536 + 77
    X, C = _rows("outlier", n, seed=1)
    Xb = pad_columns(X.to(torch.bfloat16).to(DEV))
    kvariant("assign_persist", persist)
    runs = []
    for table in (False, True):
        eng = LloydEngine(Xb, K, group_stats=table).set_centers(C.to(DEV))
        assert (eng.gstats is not None) == table
        stats = []
        for _ in range(2):
            eng.step()
            stats.append(eng.last_stats())
        runs.append((eng.C.clone(), eng.counts.clone(), eng.labels.clone(), [s.inertia for s in stats],
                     [s.n_changed for s in stats]))
    a, b = runs
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert a[3] == b[3] and a[4] == b[4]
    assert a[4][0] > 0
