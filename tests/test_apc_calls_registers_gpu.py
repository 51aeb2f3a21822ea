"""select_calls(segment, ..., registers=...) on the GPU: the trace route with register-limb constraints against the
states route fed the restatement's table, and against the second route of tests/_apc_calls_ref.py — calls, all seven counters, covered
positions and time keys."""
import numpy as np
import pytest

from tests import _apc_calls_ref as ref
from tests import _execution_states_ref as sref
from tests.test_apc_calls_gpu import same, to_apcs

pytestmark = pytest.mark.gpu
N_REGS = 8


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def named(apcs):
    return sorted({e[2] for a in apcs for c in (a[3] if len(a) > 3 else []) for e in c if e[0] == "reg"})


def expected(host, apcs, final_pc, limb_bits, initial=None):
    """the restatement's states for the registers the constraints name, as a table of N_REGS rows, and the second route on it"""
    regs = named(apcs)
    st = sref.states(host, regs, final_pc, initial_regs=None if initial is None else [initial[r] for r in regs])
    table = np.zeros((N_REGS, len(st["pcs"])), np.uint32)
    table[regs] = st["regs"]
    return st, table, ref.select(st["pcs"], apcs, regs=table.tolist(), limb_bits=limb_bits)


def check(seg, host, apcs, final_pc, limb_bits=8, initial=None, thresholds=(0,)):
    from powdr_amd import apc_calls as ac

    st, table, want = expected(host, apcs, final_pc, limb_bits, initial)
    try:
        for t in thresholds:
            ac.set_long_threshold(t)
            with ac.select_calls(seg, to_apcs(apcs), final_pc=final_pc, limb_bits=limb_bits, registers=dict(n_regs=N_REGS, initial=initial)) as got:
                same(got, want)
                assert got.time_keys == st["time_keys"] and got.n_states == len(st["pcs"])
            assert ac.last_stats()["scratch_bytes"] == 0
            with ac.select_calls(st["pcs"], to_apcs(apcs), regs=table, limb_bits=limb_bits) as by_table:
                same(by_table, want)
    finally:
        ac.set_long_threshold(0)
    return want


def limb_case(seed, n, limb_bits):
    """a state log whose registers hold few distinct words, and APCs with limb constraints: numbers, a cross-step pair of one
    register's limb, the value an instruction left (instr_idx = cycle_count), a pc"""
    rng = np.random.default_rng([seed, limb_bits])
    top = (1 << limb_bits) - 1
    words = [w & 0xFFFFFFFF for w in (0, 1, top, 1 << limb_bits, (1 << limb_bits) + 1)]
    n_limbs = min(32 // limb_bits, 2)

    def plan(i):
        return [(2 if rng.integers(0, 4) == 0 else 1, int(rng.integers(0, 4)), None if rng.integers(0, 2) else words[int(rng.integers(0, len(words)))])
                for _ in range(int(rng.integers(0, 4)))]

    ex = sref.Execution(n, seed=seed, n_regs=4, plan=plan)
    apcs = []
    for _ in range(5):
        length = int(rng.integers(1, 8))
        reg, limb = int(rng.integers(0, 4)), int(rng.integers(0, n_limbs))
        cons = [(("reg", length, reg, limb), ("reg", 0, reg, limb)),                                  # unchanged over the APC
                (("reg", length, int(rng.integers(0, 4)), 0), ("num", int(rng.integers(0, 2)))),      # what the last instruction left
                (("num", int(rng.integers(0, 2))), ("reg", int(rng.integers(0, length + 1)), int(rng.integers(0, 4)), limb)),
                (("pc", int(rng.integers(0, length + 1))), ("num", 4 * int(rng.integers(0, 5))))]
        apcs.append((4 * int(rng.integers(0, 5)), length, int(rng.integers(0, 3)), [cons[k] for k in sorted(rng.permutation(4)[:int(rng.integers(1, 4))].tolist())]))
    return ex, apcs


@pytest.mark.parametrize("limb_bits", [8, 2, 16])
def test_random_state_logs_with_limb_constraints(gpu, limb_bits):
    from tests.test_bus_check_gpu import Segment

    seen = dict.fromkeys(ref.COUNTERS, 0)
    for seed, n in ((1, 1025), (2, 300), (3, 64)):
        ex, apcs = limb_case(seed, n, limb_bits)
        host = ex.airs()
        s = Segment(gpu, host)
        try:
            want = check(s.seg, host, apcs, ex.final_pc, limb_bits, initial=ex.initial + [0] * (N_REGS - 4), thresholds=(0, 1))
        finally:
            s.close()
        for c in want["counters"]:
            for k in seen:
                seen[k] += c[k]
    assert seen["calls"] > 10 and seen["failed"] and seen["refused"] and seen["done"], seen


def test_an_off_by_one_in_p_is_seen(gpu):
    """x1 is written by every instruction to the instruction's index: the value instruction k left is k, seen at state k + 1 and not before"""
    from tests.test_bus_check_gpu import Segment

    ex = sref.Execution(60, seed=5, n_regs=2, plan=lambda i: [(1, 1, i)])
    ex.pcs[:] = [0] * 61
    rows = [(0, ts, 0, nts, acc) for _, ts, _, nts, acc in ex.rows]
    host = [(sref.state_log(rows, 3), sref.state_log_interactions(3))]
    apcs = [(0, 1, 1, [(("reg", 1, 1, 0), ("num", k))]) for k in (5, 6)] + [(0, 2, 2, [(("reg", 0, 1, 0), ("num", 9)), (("reg", 2, 1, 0), ("num", 11))])]
    s = Segment(gpu, host)
    try:
        want = check(s.seg, host, apcs, 0)
    finally:
        s.close()
    assert want["calls"] == [(0, 5, 6), (1, 6, 7), (2, 10, 12)]


def test_the_chained_execution_with_limbs_of_x2(gpu):
    """x2 counts the calls. A (one block) wants bit 0 of x2 as at the start: inserted at even calls. B (two blocks, higher priority) wants
    that bit again where its second block starts: it fails at even calls, is done at odd ones and discards the A inside it."""
    from tests import _chained_vm as vm
    from tests.test_empirical_gpu import device_airs, host_airs

    ex = vm.Execution(64, seed=3)
    n, bit = len(vm.BLOCK), ex.initial[(1, 8)][0] & 1
    apcs = [(vm.START_PC, n, 1, [(("reg", 0, 2, 0), ("num", bit))]), (vm.START_PC, 2 * n, 2, [(("reg", n, 2, 0), ("num", bit))])]
    seg, keep, _ = device_airs(gpu, ex.table, ex.rec, 64)
    try:
        want = check(seg, host_airs(ex, ex.rec), apcs, ex.end[0], limb_bits=1, thresholds=(0, 1))
    finally:
        for p, _, _ in seg:
            p.close()
    assert want["calls"] == [(0, 0, n)] + [(1, k * n, (k + 2) * n) for k in range(1, 63, 2)]
    a, b = want["counters"]
    assert a["refused"] == 32 and a["discarded"] == 31 and a["calls"] == 1 and b["failed"] == 32 and b["done"] == 31 and b["aborted"] == 2
    for key in ("refused", "failed", "done", "discarded", "calls"):
        assert any(c[key] for c in want["counters"]), key
    assert len(want["calls"]) >= 10


def test_without_a_register_literal_the_result_is_from_traces(gpu):
    from powdr_amd import apc_calls as ac
    from tests.test_bus_check_gpu import Segment

    ex = sref.Execution(300, seed=8)
    apcs = [(0, 3, 1), (4, 2, 2, [(("pc", 1), ("num", 8))]), (0, 5, 2), (8, 1, 0)]
    s = Segment(gpu, ex.airs())
    try:
        with ac.select_calls(s.seg, to_apcs(apcs), final_pc=ex.final_pc, segments=[5, 5]) as plain, \
                ac.select_calls(s.seg, to_apcs(apcs), final_pc=ex.final_pc, segments=[5, 5], registers=dict(n_regs=32)) as got:
            assert got.calls == plain.calls and got.counters == plain.counters and got.covered == plain.covered and got.time_keys == plain.time_keys
            assert len(got.calls) > 10 and got.n_states == 301
        with pytest.raises(ValueError):
            ac.select_calls(s.seg, to_apcs([(0, 1, 1, [(("reg", 0, 1, 0), ("num", 0))])]), final_pc=ex.final_pc)  # as before: no registers
        with pytest.raises(ac.ApcCallsError) as e:
            ac.select_calls(s.seg, to_apcs([(0, 1, 1, [(("reg", 0, 7, 0), ("num", 0))])]), final_pc=ex.final_pc, registers=dict(n_regs=8))
        assert (e.value.status, e.value.info) == (9, 7) and ac.last_stats()["scratch_bytes"] == 0  # (raised inside the nested stage)
    finally:
        s.close()
