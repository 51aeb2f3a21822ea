"""The signed extension arithmetic (csrc/babybear.hpp sfold / smont_any, csrc/ext.hpp bb::SExt, csrc/jit_device.hpp) without a GPU:
  * tools/ext_signed_bounds.py recomputes every range and term count from p alone; the constants the headers state (their
    `namespace bounds` blocks, static_asserted there) must be those figures;
  * tools/ext_signed_selftest_main.cpp — a program of its own, built with the host compiler and -fsanitize=address,undefined and RUN,
    not loaded into Python — drives the host forms of every operation at the edges of those ranges and on random operands against the
    unsigned bb::ext_* functions, and fills the accumulators to their allowed term counts and one fold beyond."""
import importlib.util
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


def _tool():
    spec = importlib.util.spec_from_file_location("ext_signed_bounds", ROOT / "tools" / "ext_signed_bounds.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_headers_state_the_computed_bounds():
    tool = _tool()
    stated = tool.stated_bounds()
    assert set(stated) == set(tool.computed)
    assert {k: stated[k] for k in tool.computed} == tool.computed
    assert tool.check() == len(tool.computed)
    # what the write-up quotes
    p = tool.p
    assert tool.computed["kDenTermsPerFold"] == 4 and [tool.computed[f"kAccPeriod{k}"] for k in range(4)] == [7, 3, 2, 1]
    assert tool.computed["kSmontAnyMax"] < 0.5667 * p and tool.computed["kSfoldMax"] < 0.14223 * p * p
    assert tool.computed["kMulSumMax"] <= (1 << 63) - 1 and tool.computed["kChainMax"] ** 2 <= tool.computed["kSmontDomain"]


def test_the_tool_runs_as_a_script():
    out = subprocess.run([sys.executable, str(ROOT / "tools" / "ext_signed_bounds.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "constants agree" in out.stdout, out.stdout + out.stderr


def test_host_selftest_under_the_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = tmp_path / "ext_signed_selftest"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            str(ROOT / "tools" / "ext_signed_selftest_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and "checks passed" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr, run.stderr
