"""csrc/plan_cache.hpp on the CPU: tools/plan_cache_selftest_main.cpp (header-only host code with a fake plan type that counts builds
and destructions) built with the sanitizers and run as a child process. Nothing of it is loaded into this process."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

from tests.test_poseidon2_edge_tables import SAN, _sanitizing_compiler

ROOT = Path(__file__).resolve().parent.parent
MAIN = ROOT / "tools" / "plan_cache_selftest_main.cpp"
CASES = 9  # hit, part lengths, collision, LRU, held plan, failed build, unbounded, hash, threads


def test_plan_cache_selftest_under_ubsan_and_asan(tmp_path):
    found = _sanitizing_compiler(tmp_path)
    if not found:
        pytest.skip("no host compiler with the UBSan / ASan runtimes")
    cxx, extra = found
    exe = tmp_path / "plan_cache_selftest"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-pthread", *SAN, *extra, str(MAIN), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.count(": ok") == CASES


def _tsan_compiler(tmp):
    src = tmp / "probe_tsan.cpp"
    src.write_text("int main() { return 0; }\n")
    for cxx in ("c++", "g++", "clang++"):
        exe = shutil.which(cxx)
        if not exe:
            continue
        out = tmp / "probe_tsan"
        r = subprocess.run([exe, "-fsanitize=thread", "-pthread", str(src), "-o", str(out)], capture_output=True)
        if r.returncode == 0 and subprocess.run([str(out)], capture_output=True).returncode == 0:
            return exe
    return None


def test_plan_cache_threads_under_tsan(tmp_path):
    """eight threads, four keys, a thousand lookups each: four builds and no race"""
    cxx = _tsan_compiler(tmp_path)
    if not cxx:
        pytest.skip("no host compiler with the TSan runtime")
    exe = tmp_path / "plan_cache_selftest_tsan"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=thread", str(MAIN), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([str(exe), "threads"], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.count(": ok") == 1
