"""An index that changes and lasts, on the kernels (csrc/ivf.hip: the repack beside the row pack):
the checks of tests/test_index_update.py on the GPU -- the updated index equals, bit for bit, the
index the existing build makes of the same rows -- and what only a GPU has: the fragment-packed
layout across save / load, the HBM budget and the allocator's peak against the update's plan."""
import pytest
import torch

import mikmeans
from mikmeans import ops
from mikmeans.parallel import memplan
from tests import test_index_update as T

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("d,K,off,long", T.SHAPES)
def test_add_equals_the_rebuild(native, dtype, d, K, off, long):
    got = T.check_add(DEV, dtype, d, K, off, long)
    assert got.native and got.pack.is_cuda


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_add_one_row_one_list_and_nonfinite_rows(native, dtype):
    T.check_add_batches(DEV, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("d,K,off,long", T.SHAPES)
def test_remove_equals_the_rebuild_on_the_survivors(native, dtype, d, K, off, long):
    got, _ = T.check_remove(DEV, dtype, d, K, off, long)
    assert got.native


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_remove_ignores_what_is_not_there(native, dtype):
    T.check_remove_ignores(DEV, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_add_remove_add(native, dtype):
    T.check_sequence(DEV, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_cluster_index_updates_save_and_load(native, dtype, tmp_path):
    """ClusterIndex.add / remove (device rows, and host rows in blocks of 777), the searches on the
    updated index, and the native pack through save / load; a natural-layout (CPU) index does not
    load to the GPU, nor this one to the CPU."""
    T.check_save_load(DEV, dtype, tmp_path, "cpu")
    d, K, off, long = T.SHAPES[0]
    C = T.centres(d, K)
    km = T.model_for(C, dtype)
    km.build_index(T.rows_of(C, T.add_sizes(K, off, long)[0], dtype, 1)[0]).save(tmp_path / "cpu")
    with pytest.raises(ValueError):
        mikmeans.ClusterIndex.load(tmp_path / "cpu", T.model_for(C.to(DEV), dtype))


def test_rows_wider_than_the_kernels_take_the_mirror(native):
    """D > 1024: the torch mirror on the device, natural layout, the same equalities."""
    g = torch.Generator().manual_seed(9)
    X = torch.randint(-3, 4, (300, 1100), generator=g).float().to(DEV)
    C = torch.randint(-3, 4, (4, 1100), generator=g).float().to(DEV)
    old = ops.index_build(X[:200], C)
    got = ops.index_add(old, X[200:], C)
    assert not got.native and got.pack.is_cuda
    T.assert_index_equal(got, ops.index_build(X, C))
    gone = torch.arange(0, 300, 7, device=DEV)
    mask = torch.ones(300, dtype=torch.bool)
    mask[gone.cpu()] = False
    keep = mask.nonzero().flatten()
    less, removed = ops.index_remove(got, gone)
    assert int(removed) == gone.numel()
    T.assert_index_equal(less, ops.index_build(X[keep.to(DEV)], C), keep)


def test_add_refuses_what_does_not_fit(native, monkeypatch):
    d, K, off, long = T.SHAPES[1]
    C = T.centres(d, K).to(DEV)
    km = T.model_for(C, torch.bfloat16)
    s0, s1 = T.add_sizes(K, off, long)
    X0, X1 = T.rows_of(C.cpu(), s0, torch.bfloat16, 1)[0].to(DEV), T.rows_of(C.cpu(), s1, torch.bfloat16, 2)[0].to(DEV)
    ix = km.build_index(X0)
    n0, n1 = X0.shape[0], X1.shape[0]
    plan = memplan.plan_index_update(n0, n0 + n1, d, K, "bfloat16")
    assert {k[4:]: v for k, v in plan.persistent.items() if k.startswith("old_")} == \
        {k: memplan._r(t.numel() * t.element_size()) for k, t in ix._index.tensors().items()}
    before = ix._index.tensors()
    saved = {k: t.clone() for k, t in before.items()}
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", str(plan.peak - 1))
    with pytest.raises(memplan.HBMCapacityError):
        ix.add(X1)
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", str(memplan.plan_index_update(n0, n0, d, K, "bfloat16").peak - 1))
    with pytest.raises(memplan.HBMCapacityError):
        ix.remove([0, 1])
    after = ix._index.tensors()
    assert ix.n_rows == n0 and all(after[k] is before[k] for k in before)          # the same objects,
    assert all(torch.equal(after[k].view(torch.uint8), saved[k].view(torch.uint8)) for k in before)   # the same bits
    with pytest.raises(ValueError):                                                # a wrong feature count
        ix.add(X1[:, :64])
    assert all(ix._index.tensors()[k] is before[k] for k in before)
    monkeypatch.setenv("MIKMEANS_HBM_BYTES", str(plan.peak))
    assert ix.add(X1) == n0 and ix.n_rows == n0 + n1
    assert {k: v for k, v in plan.persistent.items() if not k.startswith("old_")} == \
        {k: memplan._r(t.numel() * t.element_size()) for k, t in ix._index.tensors().items()}


def test_an_add_stays_within_its_plan(native):
    """The allocator's peak over an add of 10 % to 2 x 10^5 rows of 128 bf16 features against
    plan_index_update's (the margin of tests/test_gpu_memplan.py).  The peak is counted from the
    state before the add, which holds the old index (in the plan) and the new rows (not in it)."""
    n0, n1, d, K = 200000, 20000, 128, 256
    g = torch.Generator(device=DEV).manual_seed(0)
    C = 8.0 * torch.randn(K, d, generator=g, device=DEV)
    X = (C[torch.randint(0, K, (n0 + n1,), generator=g, device=DEV)]
         + 0.25 * torch.randn(n0 + n1, d, generator=g, device=DEV)).to(torch.bfloat16)
    km = T.model_for(C, torch.bfloat16)
    ix = km.build_index(X[:n0])
    X1 = X[n0:].clone()
    km._serving_pack(X1)                                                 # (the centre pack: built before, kept after)
    plan = memplan.plan_index_update(n0, n0 + n1, d, K, "bfloat16")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ix.add(X1)
    torch.cuda.synchronize()
    held = sum(v for k, v in plan.persistent.items() if k.startswith("old_"))   # (checked against the tensors above)
    peak = torch.cuda.max_memory_allocated() - base + held
    print("add peak", peak, "plan", plan.peak, peak / plan.peak)
    assert 0.9 * plan.peak <= peak <= 1.1 * plan.peak, (peak, plan.peak, plan.persistent, plan.transient)
