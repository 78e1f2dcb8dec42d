"""Host-code sanitizers: the native JS number formatter built with
AddressSanitizer + UndefinedBehaviorSanitizer (host only -- GPU ASan is not used), fed
random and edge-case doubles, must agree with the Python formatter byte for byte."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_jsnum_under_asan_ubsan(tmp_path):
    from mikmeans.utils.jsjson import js_number

    exe = tmp_path / "jsnum_fuzz"
    src = os.path.join(ROOT, "tests", "native", "jsnum_fuzz.cpp")
    inc = os.path.join(ROOT, "mikmeans", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", inc, src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rng = np.random.default_rng(0)
    vals = list(rng.standard_normal(3000) * 10.0 ** rng.integers(-30, 30, 3000))
    vals += list(rng.integers(0, 2**64 - 1, 3000, dtype=np.uint64).view(np.float64))
    vals += [0.0, -0.0, 1e21, 1e-7, 1e-6, 123456789012345678901.0, 5e-324, 1.7976931348623157e308,
             float("nan"), float("inf"), -float("inf"), 0.1, 1 / 3, 100.0, 1e20]
    inp = "".join(f"{struct.unpack('<Q', struct.pack('<d', float(v)))[0]:016x}\n" for v in vals)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], input=inp, capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(vals)
    for v, s in zip(vals, got):
        exp = "null" if not np.isfinite(v) else js_number(float(v))
        assert s == exp, (v, s, exp)


def _run_harness(tmp_path, name):
    """tests/native/<name>.cpp built against csrc with ASan + UBSan and run: it prints "ok <cases>"."""
    exe = tmp_path / name
    src = os.path.join(ROOT, "tests", "native", name + ".cpp")
    inc = os.path.join(ROOT, "mikmeans", "csrc")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", inc, src, "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-2000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_launch_planning_under_asan_ubsan(tmp_path):
    """csrc/plan.h (M-step slice width / LDS bytes / chunks, fixed-point exponent, assign
    Kpad) swept over K in [1, 2^20], D in [1, 256] under ASan + UBSan; the
    lanes-per-row rules pow2_at_least / pow2_at_most against the loops they replaced."""
    _run_harness(tmp_path, "plan_fuzz")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_width_dispatch_under_asan_ubsan(tmp_path):
    """csrc/dispatch.h for_width, for both element sizes: a case for exactly the widths
    plan::assign_dpad returns over D = 1..1024, every other width in 1..2048 refused; for_value:
    a case for exactly the values of its list, every other value around it refused uncalled;
    for_type: one type tag for every dtype value, bf16 for WIDTH_BF16 alone; for_flag: the flag's
    constant."""
    _run_harness(tmp_path, "width_fuzz")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_fixed_point_cell_under_asan_ubsan(tmp_path):
    """csrc/fx.h, the M-step's two-columns-per-u64 cell: n = 1, 2, FX_LIM - 1 and FX_LIM pairs at
    +-2^20 (all four sign patterns) and random in [-2^20, 2^20], added modulo 2^64, decode to both
    column sums exactly; FX_LIM + 1 adds of +2^20 do not (the no-wrap bound is tight); a label
    flushed several times (stored first, added after) totals the same."""
    _run_harness(tmp_path, "fx_fuzz")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host C++ compiler")
def test_index_walk_items_under_asan_ubsan(tmp_path):
    """csrc/walk.h, the work item of the scan, range and repack kernels: for 16, 48 and 64 pairs an
    item and random per-list pair counts (empty lists, exactly PER, PER +- 1) the items cover every
    pair once and in order, each with 1..PER pairs inside its list, their number stays within the
    grid bound walk_max_items, and list_of is right at both ends and over runs of empty lists."""
    _run_harness(tmp_path, "walk_fuzz")
