"""The persistent assign kernel's group-counter fetch and table read, in the code object (CPU:
hipcc + LLVM tools, no GPU).

csrc/assign16.hip ``assign16_persist_kernel`` takes its next row group with one returning
atomic per group, issued behind chunk 0's barrier and consumed at the last chunk's head.  It is
inline asm tied to one register, so the compiler's wait-count pass does not see it: a copy or
any other use of that register between the atomic and the kernel's own ``vmcnt(0)`` would read
it before the value landed.  This test walks every path from each such atomic to the first full
vector-memory wait and fails on any touch of its destination.  It also pins that the atomic is
not followed by a wait of its own (the round trip is what the placement hides) and that the
per-group statistics come by scalar load.
"""
import re
import shutil
from pathlib import Path

import pytest

from mikmeans import _build
from mikmeans.utils import isa

pytestmark = pytest.mark.skipif(shutil.which(_build._hipcc()) is None and not Path(_build._hipcc()).exists(),
                                reason="hipcc not available")
SRC = _build.CSRC / "assign16.hip"
NAME = "assign16_persist_kernel"
_INS = re.compile(r"^\t(?P<ins>[^/]+?)\s*//\s*(?P<addr>[0-9A-Fa-f]+):(?P<rest>.*)$")
_TARGET = re.compile(r"<[^>]*\+0x(?P<off>[0-9a-fA-F]+)>\s*$")
_FULL_WAIT = re.compile(r"s_waitcnt .*vmcnt\(0\)")


def _persist_functions(asm: str):
    """{function: [(address, instruction, branch target address or None)]} of the persistent kernels."""
    out, cur, base = {}, None, 0
    for line in asm.splitlines():
        m = re.match(r"^([0-9a-f]+) <([^>]+)>:$", line.strip())
        if m:
            cur = out.setdefault(m.group(2), []) if NAME in m.group(2) else None
            base = int(m.group(1), 16)
            continue
        if cur is None:
            continue
        m = _INS.match(line)
        if not m:
            continue
        t = _TARGET.search(m.group("rest"))
        cur.append((int(m.group("addr"), 16), m.group("ins").strip(), base + int(t.group("off"), 16) if t else None))
    return out


@pytest.fixture(scope="module")
def funcs(tmp_path_factory):
    obj = _build._compile(SRC, _build.source_flags(SRC.name), verbose=False)
    elf = isa.device_elf(obj, tmp_path_factory.mktemp("persist_counter") / "dev.o")
    fs = _persist_functions(isa.disassemble(elf))
    assert fs, "no persistent assign kernel in the code object"
    return fs


def _counter_sites(code):
    """The inline-asm fetches: returning adds on the counter word itself (the tail's arrival count is the
    compiler's own atomic, on the word after it)."""
    return [i for i, (_, ins, _) in enumerate(code)
            if ins.startswith("global_atomic_add ") and " sc0" in ins and "offset:" not in ins]


def test_counter_register_is_untouched_until_the_kernels_own_wait(funcs):
    for fn, code in funcs.items():
        index = {addr: i for i, (addr, _, _) in enumerate(code)}
        sites = _counter_sites(code)
        assert len(sites) >= 2, (fn, len(sites))   # both copies of the chunk loop (+ the one-chunk pass's)
        for s in sites:
            dest = isa._regs(isa._operands(code[s][1])[1][0])
            assert len(dest) == 1, code[s][1]
            seen, todo = set(), [s + 1]
            while todo:
                i = todo.pop()
                if i in seen:
                    continue
                seen.add(i)
                assert i < len(code), (fn, "fell off the function after", code[s][1])
                _, ins, target = code[i]
                if _FULL_WAIT.match(ins):
                    continue   # retired: this path is done
                op, ops = isa._operands(ins)
                touched = set()
                for o in ops:
                    touched |= isa._regs(o)
                assert not (touched & dest), (fn[:60], code[s][1], "then", ins)
                assert op != "s_endpgm", (fn[:60], code[s][1], "never waited for")
                if op == "s_branch":
                    todo.append(index[target])
                    continue
                if op.startswith("s_cbranch"):
                    todo.append(index[target])
                todo.append(i + 1)


def test_chunk_loop_fetch_has_no_wait_of_its_own(funcs):
    """Behind chunk 0's barrier the fetch flies under the chunk's tiles: at least two sites (the two loop
    copies) whose next vector-memory wait stands more than a tile's MFMAs away."""
    for fn, code in funcs.items():
        far = 0
        for s in _counter_sites(code):
            j = next(i for i in range(s + 1, len(code)) if re.match(r"s_waitcnt .*vmcnt\(", code[i][1]))
            far += sum(1 for _, ins, _ in code[s:j] if ins.startswith("v_mfma")) >= 16
        assert far >= 2, (fn[:60], far)


def test_group_statistics_come_by_scalar_load(funcs):
    """The table's pair is read with s_load_dwordx2 off a computed base (not the kernel arguments' s[0:1]):
    for the first group and again where the next group becomes known."""
    for fn, code in funcs.items():
        loads = [ins for _, ins, _ in code if ins.startswith("s_load_dwordx2") and not re.search(r", s\[0:1\],", ins)]
        assert len(loads) >= 2, (fn[:60], loads)
