"""APC call selection without a GPU: the second route of tests/_apc_calls_ref.py against the reference's own unit cases
(tests/golden/apc_calls_unit_cases.json), the grouping and the JSON text of `OptimisticConstraints`, the two order traps of the fold,
every refusal that needs no GPU."""
import ctypes as C
import json
from pathlib import Path

import pytest

from tests import _apc_calls_ref as ref

GOLDEN = json.loads((Path(__file__).parent / "golden" / "apc_calls_unit_cases.json").read_text())
SETS = GOLDEN["constraint_sets"]


# ---- the second route against the reference's unit cases ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GOLDEN["candidates"], ids=lambda c: c["name"])
def test_the_tracker_on_the_golden_operation_lists(case):
    apcs = [{"cycle_count": a["len"], "priority": a["priority"], "constraints": ref.Constraints(ref.constraints_from_serde(a["constraints"]))} for a in case["apcs"]]
    tracker = ref.ApcCandidates(apcs)
    pc = clk = 0
    state = lambda: (pc, (), clk)
    as_calls = lambda got: [list(c) for c in got]
    for op in case["ops"]:
        if op[0] == "insert":
            assert tracker.try_insert(state(), op[1]) == op[2], op
        elif op[0] in ("incr", "jump"):
            pc, clk = (pc + 1 if op[0] == "incr" else op[1]), clk + 1
            tracker.check_conditions(state())
            assert as_calls(tracker.extract_calls()) == op[-1], op
        elif op[0] == "counts":
            assert op[1] in (-1, tracker.count_done()) and op[2] in (-1, tracker.count_in_progress()), op
        elif op[0] == "abort":
            tracker.abort_in_progress()
        else:
            assert op[0] == "extract" and as_calls(tracker.extract_calls()) == op[1], op


@pytest.mark.parametrize("case", GOLDEN["candidates"], ids=lambda c: c["name"])
def test_the_driver_on_the_golden_executions(case):
    ex = case["execution"]
    apcs = [(start, a["len"], a["priority"], ref.constraints_from_serde(a["constraints"])) for start, a in zip(ex["start_pcs"], case["apcs"])]
    got = ref.select(ex["pcs"], apcs)
    assert [list(c) for c in got["calls"]] == ex["calls"]
    check_identities(got)


@pytest.mark.parametrize("case", GOLDEN["evaluator"], ids=lambda c: c["name"])
def test_the_evaluator_on_the_golden_cases(case):
    for run in case["runs"]:
        cons = ref.Constraints(ref.constraints_from_serde(SETS[run["constraints"]]))
        ev = ref.Evaluator(case["limb_bits"])
        for k, (s, ok) in enumerate(zip(run["states"], run["ok"])):
            assert ev.try_next_execution_step((s["pc"], tuple(s["mem"]), k), cons) == ok, (case["name"], k)


def check_identities(result):
    for c in result["counters"]:
        assert c["matches"] == c["refused"] + c["failed"] + c["aborted"] + c["done"] and c["done"] == c["discarded"] + c["calls"], c
    assert sum(c["calls"] for c in result["counters"]) == len(result["calls"])
    assert result["covered"] == sum(e - s for _, s, e in result["calls"])
    ends = [0] + [e for _, _, e in result["calls"]]
    assert all(s >= prev for (_, s, _), prev in zip(result["calls"], ends))  # in order and disjoint


# ---- the fold's order ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.TRAPS))
def test_the_order_traps(name):
    (pcs, apcs), want = ref.TRAPS[name]
    got = ref.select(pcs, apcs)
    assert got["calls"] == want
    assert [c["discarded"] for c in got["counters"]] == [1, 1, 0] and [c["done"] for c in got["counters"]] == [1, 1, 1]
    check_identities(got)


def test_batches_do_not_change_the_calls():
    """the fact DESIGN §5r builds on: one fold over all done candidates of the execution gives what the batches give"""
    import random

    rng = random.Random(5)
    for _ in range(200):
        pcs = [rng.randrange(5) for _ in range(rng.randrange(1, 40))]
        apcs = [(rng.randrange(5), rng.randrange(1, 6), rng.randrange(3), [(("pc", rng.randrange(4)), ("num", rng.randrange(5)))] if rng.random() < 0.5 else [])
                for _ in range(rng.randrange(1, 5))]
        got = ref.select(pcs, apcs)
        check_identities(got)
        # every done candidate, found directly, folded once
        table, N = ref.make_apcs(apcs), len(pcs) - 1
        done = []
        for s, pc in enumerate(pcs):
            for a, apc in enumerate(table):
                if apc["start_pc"] != pc or s + apc["cycle_count"] > N:
                    continue
                ok = all(pcs[s + step] == c[1][1] for step, cs in apc["constraints"].checks.items() if step <= apc["cycle_count"] for c in cs)
                if ok:
                    done.append((a, s, s + apc["cycle_count"]))
        tracker = ref.ApcCandidates(table)
        for a, s, e in done:
            c = ref.Candidate(a, s, None, 0)
            c.end = e
            tracker.candidates.append(c)
        assert tracker.extract_calls() == got["calls"]


# ---- OptimisticConstraints ------------------------------------------------------------------------------------------------------------------
def to_classes(cs):
    from powdr_amd import apc_calls as ac

    conv = lambda e: ac.Number(e[1]) if e[0] == "num" else ac.Pc(e[1]) if e[0] == "pc" else ac.RegisterLimb(e[1], e[2], e[3])
    return [ac.Constraint(conv(l), conv(r)) for l, r in cs]


def test_from_constraints_groups_by_step_like_the_second_route():
    from powdr_amd import apc_calls as ac

    for name, serde in SETS.items():
        tuples = ref.constraints_from_serde(serde)
        oc, want = ac.OptimisticConstraints.from_constraints(to_classes(tuples)), ref.Constraints(tuples)
        assert {k: to_classes(v) for k, v in want.checks.items()} == oc.constraints_to_check_by_step, name
        assert {k: [("Pc",) if f == ("pc",) else ("Register", f[1]) for f in v] for k, v in want.fetches.items()} == oc.fetches_by_step, name
        assert list(oc.constraints_to_check_by_step) == sorted(oc.constraints_to_check_by_step)
        assert [ac.step_of(c) for c in oc.constraints()] == sorted(ac.step_of(c) for c in oc.constraints())
    # a literal named twice is one reference; a fetch is scheduled once per constraint that needs it, not deduplicated across constraints
    oc = ac.OptimisticConstraints.from_constraints([(ac.Pc(0), ac.Pc(0)), (ac.Pc(0), ac.Pc(2)), (ac.RegisterLimb(0, 3, 1), ac.Pc(2)), (ac.Number(1), ac.Number(1))])
    assert oc.fetches_by_step == {0: [("Pc",), ("Register", 3)]} and sorted(oc.constraints_to_check_by_step) == [0, 2]
    assert oc.constraints_to_check_by_step[0] == [ac.Constraint(ac.Pc(0), ac.Pc(0)), ac.Constraint(ac.Number(1), ac.Number(1))]
    oc = ac.OptimisticConstraints.from_constraints([(ac.Pc(0), ac.Pc(1)), (ac.Pc(0), ac.Pc(2))])
    assert oc.fetches_by_step == {0: [("Pc",), ("Pc",)]}


def test_the_json_text_is_serdes():
    from powdr_amd import apc_calls as ac

    for name, want in GOLDEN["expected_json"].items():
        oc = ac.OptimisticConstraints.from_constraints(to_classes(ref.constraints_from_serde(SETS[name])))
        assert oc.to_json() == want and json.loads(oc.dumps()) == want
        assert ac.OptimisticConstraints.from_json(oc.dumps()) == oc
    for name, serde in SETS.items():
        oc = ac.OptimisticConstraints.from_constraints(to_classes(ref.constraints_from_serde(serde)))
        text = oc.to_json()
        assert [c for _, cs in sorted(text["constraints_to_check_by_step"].items(), key=lambda kv: int(kv[0])) for c in cs] == serde, name
        assert all(isinstance(k, str) and str(int(k)) == k for part in text.values() for k in part)
        assert ac.OptimisticConstraints.from_json(text) == oc
    # the empty form is what synth.py writes into an APC's JSON
    import inspect

    from powdr_amd import synth

    empty = ac.OptimisticConstraints.from_constraints([]).to_json()
    assert empty == {"fetches_by_step": {}, "constraints_to_check_by_step": {}}
    assert '"optimistic_constraints": ' + json.dumps(empty) in inspect.getsource(synth)


def test_superblock_pc_constraints():
    from powdr_amd import apc_calls as ac

    idx = ac.instruction_indexed_start_pcs([(0x100, 3), (0x200, 1), (0x100, 3)])
    assert idx == [(0, 0x100), (3, 0x200), (4, 0x100)]
    cs = ac.superblock_pc_constraints(idx)
    assert cs == [ac.Constraint(ac.Pc(0), ac.Number(0x100)), ac.Constraint(ac.Pc(3), ac.Number(0x200)), ac.Constraint(ac.Pc(4), ac.Number(0x100))]
    oc = ac.OptimisticConstraints.from_constraints(cs)
    assert oc.fetches_by_step == {} and sorted(oc.constraints_to_check_by_step) == [0, 3, 4]


# ---- refusals before any GPU call ---------------------------------------------------------------------------------------------------------
def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import apc_calls as ac
    from powdr_amd import prover

    fake = C.c_void_p(0x1000)  # never read: every call below is refused first

    def states(apcs, n_states=4, n_regs=1, limb_bits=8, pcs=fake, regs=fake, drop=None):
        t_apcs, n_apcs, t_cons, n_cons = ac.tables(apcs)
        out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
        args = [pcs, regs, n_states, n_regs, limb_bits, t_apcs, n_apcs, t_cons, n_cons, 0, C.byref(out), C.byref(status), C.byref(info)]
        if drop is not None:
            args[drop] = None
        return ac.lib.pw_apc_calls_from_states(*args)

    good = [ac.Apc(0, 2, 1, [(ac.Pc(0), ac.Number(0)), (ac.RegisterLimb(1, 0, 3), ac.Number(7))])]
    for drop in (0, 1, 5, 7, 10, 11, 12):  # a NULL pointer: pcs, registers, APCs, constraints, out, status, info
        assert states(good, drop=drop) == -1, drop
    assert states([ac.Apc(0, 0, 1)]) == -1  # cycle_count == 0
    assert states([ac.Apc(0, 1, 1, [(ac.RegisterLimb(0, 1, 0), ac.Number(0))])]) == -1  # reg >= n_regs
    assert states([ac.Apc(0, 1, 1, [(ac.RegisterLimb(0, 0, 0), ac.Number(0))])], n_regs=0) == -1
    assert states([ac.Apc(0, 1, 1, [(ac.Number(0), ac.RegisterLimb(0, 0, 4))])]) == -1  # limb * limb_bits >= 32
    assert states([ac.Apc(0, 1, 1, [(ac.RegisterLimb(0, 0, 2), ac.Number(0))])], limb_bits=16) == -1
    assert states([ac.Apc(0, 1, 1, [(ac.RegisterLimb(0, 0, 1), ac.Number(0))])], limb_bits=32) == -1
    for bits in (0, 33):
        assert states(good, limb_bits=bits) == -1
    assert states(good, n_states=1 << 32) == -1
    assert states([ac.Apc(7, 1, 1), ac.Apc(7, 2, 1)], n_states=1 << 31) == -1  # two APCs on one pc: 2^32 candidates
    # spans and kinds, on the raw tables
    t_apcs, n_apcs, t_cons, n_cons = ac.tables(good)
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    call = lambda: ac.lib.pw_apc_calls_from_states(fake, fake, 4, 1, 8, t_apcs, n_apcs, t_cons, n_cons, 0, C.byref(out), C.byref(status), C.byref(info))
    t_apcs[0].n_constraints = 3
    assert call() == -1  # a span past the array
    t_apcs[0].n_constraints, t_apcs[0].first_constraint = 1, 2
    assert call() == -1
    t_apcs[0].n_constraints, t_apcs[0].first_constraint = 2, 0
    t_cons[1].right.kind = 3
    assert call() == -1  # an unknown operand kind
    # the trace route: NULL pointers, a register literal, two segment numbers
    recs = (prover.PwSegmentAir * 2)()
    seg = (C.c_uint32 * 2)(0, 1)
    t_apcs, n_apcs, t_cons, n_cons = ac.tables([ac.Apc(0, 1, 1, [(ac.Pc(0), ac.Number(0))])])
    traces = lambda recs, n, seg, *tabs: ac.lib.pw_apc_calls_from_traces(recs, seg, n, 0, 0, *tabs, 0, C.byref(out), C.byref(status), C.byref(info))
    assert traces(None, 2, None, t_apcs, n_apcs, t_cons, n_cons) == -1
    assert traces(recs, 2, seg, t_apcs, n_apcs, t_cons, n_cons) == -1  # (a NULL prover: refused with the AIR list)
    assert traces(recs, 0, None, *ac.tables(good)) == -1  # a register literal where there are no registers
    assert ac.lib.pw_apc_calls_from_traces(recs, None, 0, 0, 0, t_apcs, n_apcs, t_cons, n_cons, 0, None, C.byref(status), C.byref(info)) == -1


def test_an_empty_execution_needs_no_gpu():
    from powdr_amd import apc_calls as ac, stage

    rc, status, info, handle = stage.raw(ac.lib.pw_apc_calls_from_states, None, None, 0, 0, 8, *ac.tables([ac.Apc(0, 2, 1), ac.Apc(4, 1, 9)]), 0)
    assert (rc, status) == (0, 0) and handle
    with ac.ApcCalls(handle) as got:
        assert got.calls == [] and got.covered == 0 and got.counters == [dict.fromkeys(ac.COUNTERS, 0)] * 2
    ac.set_long_threshold(4)
    ac.set_long_threshold(0)
    assert ac.last_stats()["candidates"] == 0 and ac.last_stats()["scratch_bytes"] == 0
