"""The signed Poseidon2 (csrc/poseidon2.hpp) under round-constant tables that are extreme WHERE THE ROUNDS CONSUME THEM: every folded
constant (ext_fold, entry_c, int_fold, exit_fold) at +-(p - 1) / 2, which is what the range analysis of tools/poseidon2_bounds.py
allows for and raw tables of equal words never produce (tests/_poseidon2_tables.py inverts derive_params). On the CPU: the derived
tables read back equal the targets exactly, the host permutation equals the oracle's, the layer-level self-test
(csrc/field_selftest.hpp, whole-permutation checks under the installed table) passes, and the same self-test runs as a program of its
own under UBSan + ASan. On the GPU: the device self-test, pw_merkle_commit on edge-valued matrices at every width around the rate,
one mixed resident / streamed LogUp segment proof with proof of work, the memory tree (Params as a kernel argument) and the Poseidon2
AIR's trace generator (its own restatement of the rounds). All arithmetic is exact: every comparison is equality."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _poseidon2_tables as tables
from tests.test_poseidon2_constants import _edge_states

P = om.P
ROOT = Path(__file__).resolve().parents[1]
TABLES = {name: (targets, E, I) for name, targets, E, I in tables.named_tables()}
GPU_TABLES = ["plus_half", "minus_half", "random_0"]


class installed:
    """the table `name` in the library and in the oracle; the placeholder again on the way out"""

    def __init__(self, name):
        self.name = name

    def __enter__(self):
        from powdr_amd import prover

        _, E, I = TABLES[self.name]
        prover.set_poseidon2_constants(E, I)
        sm.set_poseidon2_constants(E, I)
        return TABLES[self.name]

    def __exit__(self, *exc):
        from powdr_amd import prover

        prover.set_poseidon2_constants()
        sm.set_poseidon2_constants()


def host_selftest(seed, iterations):
    from powdr_amd import abi

    abi.lib.powdr_field_selftest.restype = C.c_int
    abi.lib.powdr_field_selftest.argtypes = [C.c_uint64, C.c_uint32]
    return abi.lib.powdr_field_selftest(seed, iterations)


def test_the_builder_inverts_the_scales_it_restates():
    """the targets are what they claim: every free folded constant of the first two tables is +-(p - 1) / 2, and the raw words the
    builder returns are canonical. (Equal folded constants come from raw words that are equal within a round but differ from round
    to round, as the scales do: no table of one repeated word produces them.)"""
    for name, sign in (("plus_half", 1), ("minus_half", -1)):
        t, E, I = TABLES[name]
        assert all(v == sign * tables.HALF for r in range(8) if r != 4 for v in t["ext_fold"][r])
        assert t["entry_c"] == sign * tables.HALF and set(t["int_fold"]) == {sign * tables.HALF} == set(t["exit_fold"][1:])
        assert E.shape == (8, 16) and I.shape == (13,) and int(E.max()) < P and int(I.max()) < P
        assert len(set(E.reshape(-1).tolist())) == 8 and len(set(I.tolist())) > 1


@pytest.mark.parametrize("name", list(TABLES))
def test_folded_constants_read_back_and_the_host_form_holds_under_them(name):
    from powdr_amd import prover

    with installed(name) as (targets, E, I):
        e, i, d = prover.poseidon2_constants()
        assert (e == E).all() and (i == I).all() and (d == sm.poseidon2_constants()[2]).all()
        got, want = prover.poseidon2_derived(), tables.expected_derived(targets, d)
        assert sorted(got) == sorted(want)
        for key in want:
            assert got[key] == want[key], key
        rng = np.random.default_rng(6)
        for s in list(_edge_states(rng)) + [np.full(16, (P + 1) // 2, np.uint32)]:
            assert (prover.poseidon2_host(s) == sm.poseidon2(s)).all()
        for seed in (1, 2, 0xDEADBEEF):
            assert host_selftest(seed, 2000) == 0
    z = np.zeros(16, np.uint32)
    assert (prover.poseidon2_host(z) == sm.poseidon2(z)).all()  # the placeholder is back


SAN = ["-fsanitize=undefined,address", "-fno-sanitize-recover=all"]


def _sanitizing_compiler(tmp):
    """(compiler, extra flags) that builds and runs a trivial program with the sanitizer runtimes (linked statically where possible, so
    that nothing depends on the order in which a process loads its libraries), or None"""
    src = tmp / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    for cxx in ("c++", "g++", "clang++"):
        exe = shutil.which(cxx)
        if not exe:
            continue
        for extra in (["-static-libasan", "-static-libubsan"], ["-static-libsan"], []):
            out = tmp / "probe"
            r = subprocess.run([exe, *SAN, *extra, str(src), "-o", str(out)], capture_output=True)
            if r.returncode == 0 and subprocess.run([str(out)], capture_output=True).returncode == 0:
                return exe, extra
    return None


def test_standalone_selftest_under_ubsan_and_asan(tmp_path):
    """tools/field_selftest_main.cpp (header-only: the host forms of every helper and of the permutation) built with UBSan + ASan and run
    as a child process under the placeholder and every table of this module: signed overflow in a 64-bit accumulator, the very thing
    the ranges are about, would end it. Nothing of it is loaded into this process."""
    found = _sanitizing_compiler(tmp_path)
    if not found:
        pytest.skip("no host compiler with the UBSan / ASan runtimes")
    cxx, extra = found
    exe = tmp_path / "field_selftest"
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", *SAN, *extra, str(ROOT / "tools" / "field_selftest_main.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-3000:]
    files = []
    for name, (_, E, I) in TABLES.items():
        f = tmp_path / f"{name}.txt"
        f.write_text(" ".join(str(int(w)) for w in list(E.reshape(-1)) + list(I)) + "\n")
        files.append(str(f))
    run = subprocess.run([str(exe), "2000", *files], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    assert run.stdout.count(": ok") == 1 + len(TABLES)


# ---- on the device ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import abi, prover

    return torch, abi, prover


def to_dev(torch, canonical):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(canonical, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()


def from_dev(t):
    return om.from_monty(t.cpu().numpy().view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_TABLES)
def test_device_selftest_under_the_table(gpu, name):
    torch, abi, prover = gpu
    abi.lib.powdr_field_selftest_gpu.restype = C.c_int
    abi.lib.powdr_field_selftest_gpu.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_int)]
    with installed(name):
        bad = C.c_int(-1)
        abi.check(abi.lib.powdr_field_selftest_gpu(11, 200, C.byref(bad)), "powdr_field_selftest_gpu")
        assert bad.value == 0, f"device field self-test: check {bad.value} failed"


EDGE_WIDTHS = [1, 7, 8, 9, 15, 16, 17, 23]   # one word; one short of, exactly, one past each multiple of the rate
EDGE_HEIGHTS = [2, 256, 512]                 # the smallest tree, one workgroup, two workgroups


def check_merkle_commit(gpu, height, W):
    torch, abi, prover = gpu
    d_d = torch.empty((2 * height - 1) * 8, dtype=torch.int32, device="cuda")
    for kind, m in tables.edge_matrices(height, W).items():
        _, dig = sm.merkle_commit(m, height, W, want_digests=True)
        d_m = to_dev(torch, m)
        abi.check(prover.lib.pw_merkle_commit(d_m.data_ptr(), height, W, d_d.data_ptr()), "pw_merkle_commit")
        torch.cuda.synchronize()
        assert (from_dev(d_d) == dig).all(), (kind, height, W)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["placeholder"] + GPU_TABLES)
def test_merkle_commit_of_edge_matrices_under_the_table(gpu, name):
    if name == "placeholder":
        for height in EDGE_HEIGHTS:
            for W in EDGE_WIDTHS:
                check_merkle_commit(gpu, height, W)
        return
    with installed(name):
        for height in EDGE_HEIGHTS:
            for W in EDGE_WIDTHS:
                check_merkle_commit(gpu, height, W)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_TABLES)
def test_mixed_segment_proof_under_the_table(gpu, monkeypatch, name):
    """Three AIRs of three heights, LogUp, proof of work; the 2^8-row AIR streamed (the other two are too short to stream), so the
    resident and the run-by-run leaf hashes, the strided compression with injected digests, the FRI leaves and the proof-of-work search
    all run under the table. Words == the oracle's."""
    from tests.test_segment_proof import descs_of, hip_segment, synthetic_airs

    torch, abi, prover = gpu
    airs = synthetic_airs([("T1", 200), ("T0", 3), ("T0", 2)], seed0=90)
    assert [a[2] for a in airs] == [8, 2, 1]
    monkeypatch.delenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR", raising=False)
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS", "2")
    with installed(name):
        want = sm.prove_segment(airs, num_queries=4, pow_bits=3, logup=True)
        got = hip_segment((torch, None, prover), airs, 4, 3, True)
        assert [b for b, _ in prover.segment_last_modes()] == [2, 0, 0]
        assert len(got) == len(want) and (got == want).all(), f"first differing word {int(np.argmax(got != want))} of {len(want)}"
        assert prover.verify_segment(descs_of(airs), got, 4, 3, True)[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_TABLES)
def test_memory_tree_under_the_table(gpu, name):
    """memory_tree.hip takes Params as a kernel argument, not from the constant table: a root, one update and one opening of five
    leaves at height 30 against the numpy references"""
    from powdr_amd import memory_tree as mt
    from tests import _memory_opening_ref as oref
    from tests import _memory_tree_ref as tref
    from tests.test_memory_tree_gpu import checked_update, payloads, random_keys

    torch, abi, prover = gpu
    with installed(name):
        k = prover.poseidon2_constants()
        rng = np.random.default_rng(14)
        t, want = mt.MemoryTree(30), tref.SparseTree(30, k)
        keys0 = random_keys(15, 5)
        pay0 = payloads(rng, 5)
        pay0[0], pay0[1] = P - 1, 0
        assert t.load(keys0, pay0) == (0, 0)
        want.write(keys0, pay0)
        assert (t.root() == want.root()).all()
        keys = np.unique(np.concatenate([keys0[:3], random_keys(16, 2)]))  # three stored leaves, two new ones
        init = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)
        checked_update(t, want, keys, init, payloads(rng, 5))
        status, info, pay, sib = t.open(keys)
        want_pay, want_sib = oref.opening(want, keys)
        assert (status, info) == (0, 0) and pay.shape == want_pay.shape and (pay == want_pay).all()
        assert sib.shape == want_sib.shape and (sib == want_sib).all()
        assert mt.verify_opening(30, t.root(), keys, pay, sib) == (0, 0)
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GPU_TABLES)
def test_poseidon2_air_trace_under_the_table(gpu, monkeypatch, name):
    """system_traces.hip restates the rounds for the Poseidon2 AIR's trace: six requests (edge-valued and random inputs) against the
    numpy reference, every intermediate word"""
    from powdr_amd import system_airs as sa
    from tests import _poseidon2_air_ref as ref
    from tests.test_bus_check_gpu import Segment, set_path

    torch, abi, prover = gpu
    set_path(monkeypatch, False)
    with installed(name):
        k = prover.poseidon2_constants()
        inputs = np.concatenate([np.zeros((1, 16), np.int64), np.full((1, 16), P - 1, np.int64), np.full((1, 16), (P + 1) // 2, np.int64),
                                 np.random.default_rng(1).integers(0, P, (3, 16), dtype=np.int64)])
        host = [(ref.hash_user_trace(inputs, k, 3), ref.hash_user_interactions(5))]
        want, n = ref.compress_rows(ref.requests_of(host, 5), k)
        assert n == 6 and want.shape == (ref.WIDTH, 8)
        s = Segment((torch, prover), host)
        trace, lh, rows, status = sa.poseidon2_compress_trace(s.seg, 3)
        assert (status, rows, lh) == (0, 6, 3)
        got = from_dev(trace).reshape(ref.WIDTH, 8)
        assert (got == want).all(), np.argwhere(got != want)[:5]
        s.close()
