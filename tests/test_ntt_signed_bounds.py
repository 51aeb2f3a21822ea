"""The ranges of the signed forward butterfly (bb::dit_signed in csrc/babybear.hpp, ntt::bounds in csrc/ntt.hip), on the CPU.

The integers stated in ntt::bounds are recomputed here from p alone, and tools/ntt_signed_bounds_main.cpp — a stand-alone program over
babybear.hpp's host paths, built with the host compiler (with UBSan where its runtime is there: a signed overflow in the 64-bit
accumulator is the very thing the ranges are about) — presents the butterfly with the edge grid
a, b in {0, +-1, +-(ceil(B p) - 1)}, w, kappa in {+-(p - 1) / 2, +-1, 0} and with 10^6 random triples: |t| inside the reduction's
domain, every output below the stated bound, X = a + b w and Y = a - b w (mod p) against plain 64-bit modular arithmetic."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
P = 2013265921
B = 1  # ntt::bounds states the ranges for |a|, |b| < B p with B = 1 (canonical inputs are inside; the outputs close below it)


def _stated():
    text = (ROOT / "powdr_amd" / "csrc" / "ntt.hip").read_text()
    block = re.search(r"namespace ntt \{\nnamespace bounds \{\n(.*?)\n\}  // namespace bounds", text, re.S).group(1)
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int64_t (k\w+) = (-?\d+)ll;", block)}


def _recomputed():
    domain = 2**63 - 2**31 * P            # bb::smont: |t| + 2^31 p < 2^63
    in_top = -(-B * P // 1)                # ceil(B p), exclusive
    tw_top = (P - 1) // 2                  # centred twiddles and kappa, inclusive
    wide_top = 2 * (in_top - 1) * tw_top   # |a kappa + b w|, inclusive
    out_top = (wide_top + 2**31 * P) // 2**32 + 1  # |(t + m p) / 2^32| with m in [-2^31, 2^31), exclusive
    return {"kSmontDomain": domain, "kInTop": in_top, "kTwiddleTop": tw_top, "kWideTop": wide_top, "kOutTop": out_top}


def test_stated_bounds_are_the_recomputed_ones():
    stated, want = _stated(), _recomputed()
    assert stated == want
    assert want["kWideTop"] < want["kSmontDomain"]          # inside the reduction's domain
    assert want["kOutTop"] <= want["kInTop"]                # the range closes from one stage to the next
    assert want["kOutTop"] < (0.469 * B + 0.5) * P          # the bound in its closed form
    assert want["kOutTop"] + P <= 2**32                     # the store's x + p does not wrap
    assert 2**32 % P <= want["kTwiddleTop"]                 # kappa = R mod p is centred as it stands


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ntt_signed_bounds")
    cxx = next((shutil.which(c) for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    src = ROOT / "tools" / "ntt_signed_bounds_main.cpp"
    exe = tmp / "ntt_signed_bounds"
    err = ""
    for san in (["-fsanitize=undefined", "-fno-sanitize-recover=all"], []):
        build = subprocess.run([cxx, "-std=c++17", "-O1", *san, str(src), "-o", str(exe)], capture_output=True, text=True)
        if build.returncode == 0 and subprocess.run([str(exe)], capture_output=True).returncode == 2:  # its usage line
            return exe
        err = build.stderr
    raise AssertionError(err[-3000:])


def _run(exe, b, n_random):
    run = subprocess.run([str(exe), *(str(b[k]) for k in ("kInTop", "kTwiddleTop", "kSmontDomain", "kOutTop")), str(n_random)],
                         capture_output=True, text=True, timeout=120)
    return run.returncode, run.stdout + run.stderr


def test_butterfly_at_the_edges_and_on_random_triples(program):
    b = _stated()
    rc, out = _run(program, b, 10**6)
    assert rc == 0, out[-3000:]
    got = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", out)}
    assert got["checked"] == 5**4 + 10**6
    # the grid reaches the stated range of t: |t| = (p - 1)^2 exactly
    assert got["edge_max_wide"] == b["kWideTop"]
    assert got["edge_max_out"] < b["kOutTop"] and got["max_out"] < b["kOutTop"]
    assert got["max_wide"] <= b["kWideTop"]


def test_program_refuses_a_range_that_does_not_hold(program):
    """The checks are live: the grid's edge a = b = p - 1, w = kappa = (p - 1) / 2 gives |t| = kWideTop exactly, so a domain that ends
    there (exclusive) is left."""
    b = dict(_stated())
    b["kSmontDomain"] = b["kWideTop"]
    rc, out = _run(program, b, 0)
    assert rc == 1 and "FAILED" in out
