"""Register budget and in-flight-register guard of the persistent assign kernel (CPU: hipcc +
LLVM tools, no GPU).

csrc/assign16.hip ``assign16_persist_kernel`` reloads the next row group's fragments into the
registers that hold the current ones, under the label epilogue.  That only pays while the
kernel keeps the one-pass kernel's occupancy (4 waves/SIMD: 128 VGPRs) without a spill -- a
second fragment set spilled inside the chunk loop and ran 13-15 % slower
(profiles/r4_04_persistent_grid_ab.md) -- and it is only correct while nothing but the loads
and the MFMAs touches those registers: the loads are inline asm the compiler's wait-count pass
does not see, so a copy or a spill of a fragment register would read it before it landed.
"""
import re
import shutil
from collections import Counter
from pathlib import Path

import pytest

from mikmeans import _build
from mikmeans.utils import isa

pytestmark = pytest.mark.skipif(shutil.which(_build._hipcc()) is None and not Path(_build._hipcc()).exists(),
                                reason="hipcc not available")
SRC = _build.CSRC / "assign16.hip"
NAME = "assign16_persist_kernel"
# VGPRs a kernel may hold at its launch-bounds occupancy (waves per SIMD), 512 per SIMD lane
BUDGET = {4: 128, 3: 168}


@pytest.fixture(scope="module")
def elf(tmp_path_factory):
    obj = _build._compile(SRC, _build.source_flags(SRC.name), verbose=False)
    return isa.device_elf(obj, tmp_path_factory.mktemp("persist") / "dev.o")


def _template_ints(demangled: str) -> list[int]:
    inner = demangled[demangled.index(NAME + "<") + len(NAME) + 1:]
    return [int(x) for x in inner[: inner.index(">")].split(",")]


def test_persistent_instantiations_fit_their_occupancy_without_spills(elf):
    res = [r for r in isa.kernel_resources(elf) if NAME in r.name]
    assert res, "no persistent assign kernel in the code object"
    for r in res:
        dpad, p, occ, pmaj = _template_ints(r.name)
        assert occ in BUDGET, r.name
        assert r.vgprs <= BUDGET[occ], (r.name, r.vgprs)
        assert r.vgpr_spills == 0 and r.scratch_bytes == 0, (r.name, r.vgpr_spills, r.scratch_bytes)
    # the headline geometry is among them: bf16 D=128, 4 point blocks, 4 waves/SIMD, block-major issue
    assert any(_template_ints(r.name) == [128, 4, 4, 1] for r in res), [r.name for r in res]


def test_persistent_kernel_seeds_are_scalar_adds(elf):
    """The per-tile seed-offset add feeds the MFMAs' srcC: never a packed-f32 write (see
    tests/test_isa_guard.py)."""
    funcs = isa.functions(isa.disassemble(elf))
    assert any(NAME in f for f in funcs)
    hz = isa.packed_seed_hazards(funcs, name_filter=NAME)
    assert not hz, [(h.function[:60], h.writer, h.mfma) for h in hz[:5]]


def test_fragment_registers_are_touched_by_loads_and_mfmas_only(elf):
    """From the first fragment load on, the fragment registers appear only as the destination of
    the two load sites (first group, prefetch under the epilogue: the same registers) and as MFMA
    operands: no copy, no spill, no reuse while a load may be in flight."""
    funcs = isa.functions(isa.disassemble(elf))
    mine = {f: ls for f, ls in funcs.items() if NAME in f}
    assert mine
    for fn, lines in mine.items():
        loads = [i for i, x in enumerate(lines) if x.startswith("global_load_dwordx4")]
        assert loads, fn
        dests = Counter(lines[i].split(None, 1)[1].split(",")[0].strip() for i in loads)
        assert set(dests.values()) == {2}, dests   # every tuple loaded at both sites
        frag = set()
        for d in dests:
            frag |= isa._regs(d)
        assert len(frag) == 4 * len(dests)
        # the kernel's tail (past the group loop: its last barrier, MFMA and load) starts with a
        # full wait; behind it the registers are free again
        last = max(i for i, x in enumerate(lines) if x.startswith(("v_mfma", "global_load_dwordx4", "s_barrier")))
        tail = next(i for i in range(last + 1, len(lines)) if re.match(r"s_waitcnt vmcnt\(0\)", lines[i]))
        issued = set()   # fragment registers whose first load is out: from then on, loads and MFMAs only
        for x in lines[loads[0]:tail]:
            op, ops = isa._operands(x)
            touched = set()
            for o in ops:
                touched |= isa._regs(o)
            if op.startswith("global_load_dwordx4"):
                assert not (set().union(*(isa._regs(o) for o in ops[1:])) & issued), x   # (its address)
                issued |= isa._regs(ops[0])
                continue
            if not (touched & issued):
                continue
            assert op.startswith("v_mfma"), (fn[:60], x)
            # a fragment is the MFMA's B operand only, never its destination or accumulator
            assert not ((isa._regs(ops[0]) | isa._regs(ops[3])) & issued), x
        assert issued == frag
        # and the kernel waits for them itself: a full wait before each group's offset reduction
        # and each chunk's barrier; the label epilogue's counted wait leaves them in flight
        waits = [x for x in lines if re.match(r"s_waitcnt .*vmcnt\(", x)]
        assert any("vmcnt(17)" in w for w in waits) and any("vmcnt(0)" in w for w in waits), waits
