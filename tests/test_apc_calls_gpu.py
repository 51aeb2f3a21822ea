"""pw_apc_calls_from_states / _from_traces on the GPU against the second route of tests/_apc_calls_ref.py: the calls in
order, every counter of every APC and the covered positions, exactly."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _apc_calls_ref as ref
from tests import _empirical_ref as eref

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).parent / "golden" / "apc_calls_unit_cases.json").read_text())
SETS = GOLDEN["constraint_sets"]
SIZES = [0, 1, 2, 63, 64, 65, 1025, 2**16 + 1]  # N instructions: N + 1 states
P = 0x100                                       # the two-instruction block of the self-loop: pcs P, P + 4
LOOP_A = (P, 2, 1, [(("pc", 0), ("num", P))])
LOOP_AA = (P, 4, 2, [(("pc", 0), ("num", P)), (("pc", 2), ("num", P))])


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def to_apcs(apcs):
    from powdr_amd import apc_calls as ac

    conv = lambda e: ac.Number(e[1]) if e[0] == "num" else ac.Pc(e[1]) if e[0] == "pc" else ac.RegisterLimb(e[1], e[2], e[3])
    return [ac.Apc(a[0], a[1], a[2], [ac.Constraint(conv(l), conv(r)) for l, r in (a[3] if len(a) > 3 else [])]) for a in apcs]


def same(got, want):
    assert [tuple(c) for c in got.calls] == want["calls"]
    assert got.counters == want["counters"] and got.covered == want["covered"]
    for c in got.counters:
        assert c["matches"] == c["refused"] + c["failed"] + c["aborted"] + c["done"] and c["done"] == c["discarded"] + c["calls"], c


def check(gpu, pcs, apcs, regs=None, limb_bits=8, want=None, **kw):
    """the device result compared field by field with the second route (computed once per input by the caller where it is shared)"""
    from powdr_amd import apc_calls as ac

    want = want or ref.select(pcs, apcs, regs=regs, limb_bits=limb_bits)
    with ac.select_calls(pcs, to_apcs(apcs), regs=regs, limb_bits=limb_bits, **kw) as got:
        same(got, want)
        assert got.n_states == len(pcs) and got.time_keys == []
    stats = ac.last_stats()
    assert stats["scratch_bytes"] == 0 and stats["valid"] == sum(c["done"] for c in want["counters"])
    assert stats["candidates"] == sum(c["matches"] for c in want["counters"])
    return want, stats


@pytest.fixture
def thresholds():
    """runs f under the default threshold and under small ones that send short components down the long path; always restored"""
    from powdr_amd import apc_calls as ac

    def run(f, values=(0, 1, 4)):
        try:
            out = []
            for t in values:
                ac.set_long_threshold(t)
                out.append(f())
            return out
        finally:
            ac.set_long_threshold(0)

    return run


# ---- the reference's unit cases, the traps --------------------------------------------------------------------------------------------------
def test_the_golden_executions(gpu, thresholds):
    for case in GOLDEN["candidates"]:
        ex = case["execution"]
        apcs = [(start, a["len"], a["priority"], ref.constraints_from_serde(a["constraints"])) for start, a in zip(ex["start_pcs"], case["apcs"])]
        want = ref.select(ex["pcs"], apcs)
        assert [list(c) for c in want["calls"]] == ex["calls"], case["name"]
        thresholds(lambda: check(gpu, ex["pcs"], apcs, want=want))


def test_the_golden_evaluator_cases_as_executions(gpu):
    """every run as one APC over its states (a run of one state gets a second state, which no constraint reads): done or not as `ok` says"""
    for case in GOLDEN["evaluator"]:
        for run in case["runs"]:
            states = run["states"] + ([run["states"][0]] if len(run["states"]) == 1 else [])
            pcs = [s["pc"] for s in states]
            regs = [[s["mem"][r] for s in states] for r in range(2)]
            apcs = [(pcs[0], len(states) - 1, 1, ref.constraints_from_serde(SETS[run["constraints"]]))]
            want, _ = check(gpu, pcs, apcs, regs=regs, limb_bits=case["limb_bits"])
            assert want["counters"][0]["done"] == int(all(run["ok"])), case["name"]


@pytest.mark.parametrize("name", sorted(ref.TRAPS))
def test_the_order_traps(gpu, thresholds, name):
    (pcs, apcs), calls = ref.TRAPS[name]
    for want, stats in thresholds(lambda: check(gpu, pcs, apcs)):
        assert want["calls"] == calls and stats["components"] == 1 and stats["longest_component"] == 3
    assert [s["long_components"] for _, s in thresholds(lambda: check(gpu, pcs, apcs))] == [0, 1, 0]


# ---- random executions ------------------------------------------------------------------------------------------------------------------------
def random_case(rng, n, n_regs=2, limb_bits=8):
    """n instructions over a pc alphabet of 5; 1 to 6 APCs of length 1 to 9 with tied priorities and lengths and shared start pcs; constraints
    over pcs and register limbs, numbers, cross-step pairs, a constant-false pair (never inserted), a literal beyond cycle_count (ignored)"""
    pcs = (4 * rng.integers(0, 5, size=n + 1)).tolist()
    n_limbs = 32 // limb_bits
    top = (1 << limb_bits) - 1
    words = [w & 0xFFFFFFFF for w in (0, 1, top, 1 << limb_bits, (1 << limb_bits) + 1)]
    regs = [[words[i] for i in rng.integers(0, len(words), size=n + 1)] for _ in range(n_regs)]
    apcs = []
    for _ in range(int(rng.integers(1, 7))):
        length = int(rng.integers(1, 10))
        lit = lambda hi: (("pc", int(rng.integers(0, hi + 1))) if rng.integers(0, 2) else
                          ("reg", int(rng.integers(0, hi + 1)), int(rng.integers(0, n_regs)), int(rng.integers(0, min(n_limbs, 2)))))
        cons = []
        for _ in range(int(rng.integers(0, 4))):
            kind = int(rng.integers(0, 6))
            if kind == 0:
                cons.append((("pc", int(rng.integers(0, length + 1))), ("num", 4 * int(rng.integers(0, 5)))))
            elif kind == 1:
                cons.append((("num", int(rng.integers(0, 2))), ("reg", int(rng.integers(0, length + 1)), int(rng.integers(0, n_regs)), int(rng.integers(0, min(n_limbs, 2))))))
            elif kind == 2:
                cons.append((lit(length), lit(length)))  # a cross-step pair (or one state twice)
            elif kind == 3:
                cons.append((("num", 1), ("num", 2)) if rng.integers(0, 4) == 0 else (("num", 7), ("num", 7)))
            elif kind == 4:
                cons.append((("pc", length + 1 + int(rng.integers(0, 3))), ("num", 12345)))  # beyond cycle_count: never checked
            else:
                cons.append((("pc", 0), ("pc", int(rng.integers(0, length + 1)))))
        apcs.append((4 * int(rng.integers(0, 5)), length, int(rng.integers(0, 3)), cons))
    return pcs, regs, apcs


@pytest.mark.parametrize("n", SIZES)
def test_random_executions(gpu, thresholds, n):
    rng = np.random.default_rng(n + 17)
    seen = dict.fromkeys(ref.COUNTERS, 0)
    for rep in range(1 if n > 2000 else 6):
        limb_bits = (8, 2, 8, 16, 32, 8)[rep]
        pcs, regs, apcs = random_case(rng, n, limb_bits=limb_bits)
        want = ref.select(pcs, apcs, regs=regs, limb_bits=limb_bits)
        thresholds(lambda: check(gpu, pcs, apcs, regs=regs, limb_bits=limb_bits, want=want), values=(0, 4) if n > 2000 else (0, 1, 4))
        for c in want["counters"]:
            for k in seen:
                seen[k] += c[k]
    if n == 1025:
        assert all(seen.values()), seen  # every outcome occurs among the six cases of this size


def test_no_registers_and_no_apcs(gpu):
    from powdr_amd import apc_calls as ac

    want, stats = check(gpu, [0, 4, 8, 0, 4], [])
    assert want["calls"] == [] and stats["candidates"] == 0
    want, _ = check(gpu, [0, 4, 8, 0, 4], [(0, 1, 1), (4, 1, 1)])
    assert want["calls"] == [(0, 0, 1), (1, 1, 2), (0, 3, 4)] and want["counters"][1]["aborted"] == 1
    with ac.select_calls([], to_apcs([(0, 1, 1)])) as got:
        assert got.calls == [] and got.n_states == 0
    with pytest.raises(ValueError):
        ac.select_calls([0, 4], to_apcs([(0, 1, 1, [(("reg", 0, 0, 0), ("num", 0))])]))  # a register literal without registers


def test_limbs_at_8_and_2_bits(gpu):
    # x = 0b10110110 = 182: 2-bit limbs 2, 1, 3, 2; 8-bit limbs of 0x04030201
    pcs, regs = [0, 4, 0, 4, 0], [[182, 0, 182, 0, 183], [0x04030201] * 5]
    two = [(0, 1, 1, [(("reg", 0, 0, k), ("num", v)) for k, v in enumerate([2, 1, 3, 2])] + [(("reg", 0, 1, 15), ("num", 0))])]
    want, _ = check(gpu, pcs, two, regs=regs, limb_bits=2)
    assert want["calls"] == [(0, 0, 1), (0, 2, 3)] and want["counters"][0]["refused"] == 1  # (183 differs in limb 0)
    eight = [(0, 2, 1, [(("reg", 1, 1, k), ("num", k + 1)) for k in range(4)] + [(("reg", 0, 0, 0), ("reg", 2, 0, 0))])]
    want, _ = check(gpu, pcs, eight, regs=regs, limb_bits=8)
    assert want["calls"] == [(0, 0, 2)] and want["counters"][0]["failed"] == 1 and want["counters"][0]["aborted"] == 1


def test_one_constraint_next_to_4096(gpu):
    rng = np.random.default_rng(4)
    n = 200
    pcs = (4 * rng.integers(0, 2, size=n + 1)).tolist()
    regs = [rng.integers(0, 3, size=n + 1).tolist()]
    big = [(("pc", k % 3), ("pc", k % 3)) if k % 5 else (("num", k), ("num", k)) for k in range(4094)]
    big += [(("reg", 1, 0, 0), ("num", 1)), (("reg", 0, 0, 0), ("reg", 2, 0, 0))]  # the last chunk decides
    apcs = [(0, 2, 1, [(("pc", 1), ("num", 4))]), (0, 3, 2, big), (4, 1, 1, [])]
    want, _ = check(gpu, pcs, apcs, regs=regs)
    c = want["counters"][1]
    assert c["done"] > 0 and c["failed"] > 0 and c["refused"] == 0 and want["counters"][0]["calls"] > 0


# ---- the hot loop ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop():
    iterations = 1 << 15
    pcs = [P, P + 4] * iterations + [P]
    return pcs, {"both": ref.select(pcs, [LOOP_A, LOOP_AA]), "a": ref.select(pcs, [LOOP_A])}, iterations


def test_the_self_loop_is_one_component(gpu, thresholds, loop):
    pcs, wants, iterations = loop
    want = wants["both"]
    assert want["calls"] == [(1, 4 * k, 4 * k + 4) for k in range(iterations // 2)]  # AA at every fourth position
    for _, stats in thresholds(lambda: check(gpu, pcs, [LOOP_A, LOOP_AA], want=want), values=(0, 4)):
        assert stats["components"] == 1 and stats["long_components"] == 1
        assert stats["longest_component"] == stats["valid"] == 2 * iterations - 1
    # the final state starts an A and an AA that the end aborts, and so is the AA of the last iteration
    assert want["counters"][0]["aborted"] == 1 and want["counters"][1]["aborted"] == 2 and want["covered"] == 2 * iterations


def test_the_loop_with_a_alone_is_components_of_one(gpu, loop):
    pcs, wants, iterations = loop
    want, stats = check(gpu, pcs, [LOOP_A], want=wants["a"])
    assert want["calls"] == [(0, 2 * k, 2 * k + 2) for k in range(iterations)]
    assert stats["components"] == stats["valid"] == iterations and stats["longest_component"] == 1 and stats["long_components"] == 0


def test_a_dense_component_crosses_the_staged_stretch(gpu, thresholds):
    """one pc, six APCs of up to 20 instructions: one component of thousands of candidates in which a candidate meets more than a wave
    of followers, across the boundaries of the stretch the long path stages"""
    rng = np.random.default_rng(9)
    pcs = [0] * 1026
    apcs = [(0, int(rng.integers(1, 21)), int(rng.integers(0, 3))) for _ in range(5)] + [(0, 20, 1)]
    want = ref.select(pcs, apcs)
    for _, stats in thresholds(lambda: check(gpu, pcs, apcs, want=want), values=(0, 4)):
        assert stats["components"] == 1 and stats["long_components"] == 1 and stats["longest_component"] > 4096


def test_candidates_cut_off_by_the_end(gpu):
    want, _ = check(gpu, [0, 4, 8], [(0, 4, 1), (0, 2, 1), (8, 1, 5), (4, 2, 1, [(("pc", 1), ("num", 9))])])
    assert want["calls"] == [(1, 0, 2)]
    assert [c["aborted"] for c in want["counters"]] == [1, 0, 1, 0] and want["counters"][3]["failed"] == 1


# ---- scratch ----------------------------------------------------------------------------------------------------------------------------------
def test_status_2_and_the_bytes_it_names(gpu):
    from powdr_amd import apc_calls as ac

    rng = np.random.default_rng(21)
    pcs, regs, apcs = random_case(rng, 3000)
    with pytest.raises(ac.ApcCallsError) as e:
        ac.select_calls(pcs, to_apcs(apcs), regs=regs, scratch_bytes=1)
    assert e.value.status == 2 and e.value.info > 1 and "bytes needed" in str(e.value) and ac.last_stats()["scratch_bytes"] == 0
    _, stats = check(gpu, pcs, apcs, regs=regs, scratch_bytes=e.value.info)
    assert 0 < stats["peak_bytes"] <= e.value.info
    with pytest.raises(ac.ApcCallsError) as again:
        ac.select_calls(pcs, to_apcs(apcs), regs=regs, scratch_bytes=e.value.info - 1)
    assert again.value.status == 2 and again.value.info == e.value.info


# ---- the trace route --------------------------------------------------------------------------------------------------------------------------
def traces_of(gpu, logs, apcs, final_pc, segments=None, **kw):
    from powdr_amd import apc_calls as ac
    from tests.test_bus_check_gpu import Segment

    s = Segment(gpu, logs)
    try:
        return ac.select_calls(s.seg, to_apcs(apcs), final_pc=final_pc, segments=segments, **kw)
    finally:
        s.close()


def test_traces_in_any_row_order_equal_the_pc_list(gpu):
    rng = np.random.default_rng(3)
    pcs, _, _ = random_case(rng, 300)
    apcs = [(0, 3, 1), (4, 2, 2, [(("pc", 1), ("num", 8))]), (0, 5, 2), (8, 1, 0)]
    rows = [[], []]
    for t, pc in enumerate(pcs[:-1]):
        rows[t % 2].append((pc, 100 + 3 * t, [t]))
    it = eref.block_log_interactions()
    logs = [(eref.block_log(r, 1, log_h=9, places=rng.permutation(1 << 9)[:len(r)]), it) for r in rows]
    want = ref.select(pcs, apcs)
    with traces_of(gpu, logs, apcs, pcs[-1], segments=[5, 5]) as got:
        same(got, want)
        assert got.n_states == len(pcs) and got.time_keys == [(5 << 32) | (100 + 3 * t) for t in range(len(pcs) - 1)]
    assert len(want["calls"]) > 10


def test_trace_statuses(gpu):
    from powdr_amd import apc_calls as ac

    it = eref.block_log_interactions()
    rows = [(pc, 10 + t, [0]) for t, pc in enumerate([0, 4, 8, 0])]
    log = lambda rs: [(eref.block_log(rs, 1), it)]
    apcs = [(0, 2, 1)]
    with traces_of(gpu, log(rows), apcs, 4) as got:
        assert [tuple(c) for c in got.calls] == [(0, 0, 2)] and got.counters[0]["aborted"] == 1
    with pytest.raises(ac.ApcCallsError) as e:  # 4: a duplicate time key
        traces_of(gpu, log(rows + [(4, 12, [0])]), apcs, 4)
    assert (e.value.status, e.value.info) == (4, 12) and ac.last_stats()["scratch_bytes"] == 0  # (raised after the index stage allocated)
    twice = eref.block_log(rows, 1)
    twice[0, 3] = 2
    with pytest.raises(ac.ApcCallsError) as e:  # 7: a multiplicity of 2, the smallest (air, row)
        traces_of(gpu, log(rows) + [(twice, it)], apcs, 4)
    assert (e.value.status, e.value.info) == (7, (1 << 32) | 3) and ac.last_stats()["scratch_bytes"] == 0
    with pytest.raises(ValueError):  # -1: two segment numbers
        traces_of(gpu, log(rows) + log(rows), apcs, 4, segments=[0, 1])
    with pytest.raises(ac.ApcCallsError) as e:
        traces_of(gpu, log(rows), apcs, 4, scratch_bytes=1)
    assert e.value.status == 2
    with traces_of(gpu, log(rows), apcs, 4, scratch_bytes=e.value.info) as got:
        assert len(got.calls) == 1 and ac.last_stats()["peak_bytes"] <= e.value.info and ac.last_stats()["scratch_bytes"] == 0
    with traces_of(gpu, log(rows), apcs, 0, bus=1) as got:  # no AIR on the bus: the final state alone
        assert got.calls == [] and got.n_states == 1 and got.counters[0]["aborted"] == 1


def test_the_chained_execution_with_superblock_apcs(gpu):
    """§5j's execution: the APCs are the superblocks `execution_blocks.detect` finds in the same traces, with the pc constraints of
    `superblock_pc_constraints`; the trace route equals the pc route and the second route"""
    from powdr_amd import apc_calls as ac
    from powdr_amd import execution_blocks as eb
    from tests import _chained_vm as vm
    from tests.test_empirical_gpu import device_airs

    ex = vm.Execution(64, seed=3)
    n = len(vm.BLOCK)
    pcs = [vm.START_PC + 4 * i for i in range(n)] * 64 + [ex.end[0]]
    seg, keep, _ = device_airs(gpu, ex.table, ex.rec, 64)
    try:
        with eb.detect(seg, [(vm.START_PC, n)], max_bb=3) as blocks:
            supers = [s for s, _ in blocks.blocks()]
        assert supers == [(vm.START_PC,) * k for k in (1, 2, 3)]
        apcs, tuples = [], []
        for s in supers:
            cons = ac.superblock_pc_constraints(ac.instruction_indexed_start_pcs([(pc, n) for pc in s]))
            apcs.append(ac.Apc(s[0], n * len(s), len(s), cons))
            tuples.append((s[0], n * len(s), len(s), [(("pc", c.left.instr_idx), ("num", c.right.value)) for c in cons]))
        want = ref.select(pcs, tuples)
        with ac.select_calls(seg, apcs, final_pc=ex.end[0]) as got, ac.select_calls(pcs, apcs) as by_pcs:
            same(got, want)
            same(by_pcs, want)
            assert len(got.time_keys) == 64 * n and got.time_keys == sorted(got.time_keys)
        assert want["calls"] == [(2, 3 * n * k, 3 * n * (k + 1)) for k in range(21)] + [(0, 63 * n, 64 * n)] and want["covered"] == 64 * n
    finally:
        for p, _, _ in seg:
            p.close()
