"""The three system AIRs that close a segment's buses (powdr_amd/system_airs.py), no GPU: on a chained execution
(tests/_chained_vm.py) with the instruction-chip rows of the library's own expanders and the reference system traces
(tests/_system_airs_ref.py) every constraint of the three AIRs vanishes and all six buses balance tuple by tuple; each of four
mutations breaks the constraint or the bus it should."""
import numpy as np
import pytest

from oracle import original_chips as ooc
from tests import _bus_multiset as bm
from tests import _chained_vm as vm
from tests import _system_airs_ref as ref

P = ooc.P
CALLS = 64
ALL_BUSES = (0, 1, 2, 3, 6, 7)


def host_expanded_airs(ex):
    """the instruction AIRs of the execution, every row by powdr_original_row_expand_host (the library's expander code on the host)"""
    from powdr_amd import original_chips as pc
    from powdr_amd import synth

    t = pc.InstructionTable(ex.block, [True] * len(ex.block), ex.start_pc)
    traces = {}
    for entry, row in zip(t.entries, ex.table):
        k, o, n = int(row["kind"]), int(row["rec_off"]), ooc.RECORD_WORDS[int(row["kind"])]
        rows = ex.rbs[k] * ex.calls
        tr = traces.setdefault(k, np.zeros((ooc.WIDTHS[k], max(4, 1 << (rows - 1).bit_length())), np.uint32))
        for r in range(ex.calls):
            tr[:, int(row["air_row"]) + r * ex.rbs[k]] = pc.expand_row_host(entry, ex.rec[o:o + n, r], int(ex.rec[0, r]) + int(row["ts_delta"]))
    return [(ooc.KIND_NAMES[k], tr, synth.reference_air_programs(ooc.KIND_NAMES[k])) for k, tr in sorted(traces.items())]


@pytest.fixture(scope="module")
def closed():
    from powdr_amd import system_airs as sa

    ex = vm.Execution(CALLS, seed=3)
    instr = host_expanded_airs(ex)
    assert len(instr) >= 5 and {"LoadStore", "BaseAlu", "JalLui"} <= {n for n, _, _ in instr}
    assert [(n, t.tolist()) for n, t, _ in instr] == [(n, t.tolist()) for n, t, _ in ex.instruction_airs()]  # = the numpy restatement
    for name, t, (bc, sp, _) in instr:  # the chips' own constraints hold on the chained records
        assert ooc.check_constraints(bc, sp, [t[c] for c in range(t.shape[0])])[0] == 0, name
    senders = [(t, programs[2]) for _, t, programs in instr]
    table = ex.program_table()
    airs = dict(program=sa.program_air(table), connector=sa.connector_air(), boundary=sa.boundary_air())
    truth = (ref.program_freq(table, {ex.start_pc + 4 * i: CALLS for i in range(len(ex.block))}), ref.connector_trace(ex.start, ex.end),
             ref.boundary_trace(ex.initial, ex.final))
    return dict(ex=ex, senders=senders, table=table, airs=airs, traces=dict(zip(("program", "connector", "boundary"), truth)))


def segment(closed, traces=None):
    """[(cols, interactions)] of the closed segment: senders, the three system AIRs (main | preprocessed columns), and the periphery
    AIRs that receive every lookup of both"""
    tr = dict(closed["traces"], **(traces or {}))
    a = closed["airs"]
    system = [(np.concatenate([tr["program"], closed["table"]]), a["program"].inter),
              (np.concatenate([tr["connector"], a["connector"].fixed]), a["connector"].inter), (tr["boundary"], a["boundary"].inter)]
    open_airs = closed["senders"] + system
    return open_airs + ref.periphery_airs(bm.tally(open_airs)[0])


def unbalanced(airs):
    table, active = bm.tally(airs)
    return {bus: sorted(k[2] for k, e in table.items() if e[0] and k[0] == bus) for bus in active}


def test_the_block_is_what_the_issue_asks_for(closed):
    ex = closed["ex"]
    kinds = {int(r["kind"]) for r in ex.table}
    assert len(kinds) >= 5
    ops = [int(r["opcode"]) for r in ex.table]
    assert 528 in ops and 531 in ops and all(int(r["e"]) == 2 for r in ex.table if int(r["opcode"]) in (528, 531))
    assert ops[-1] == 560 and (ex.start_pc + 4 * (len(ops) - 1) + int(ex.table[-1]["c"])) % P == ex.start_pc  # JAL x0 back to the first pc
    # call k + 1 starts at call k's end timestamp, and x2 is written in one call and read in the next
    step = sum(ooc.TS_STEP[int(r["kind"])] for r in ex.table)
    assert (np.diff(ex.rec[0].astype(np.int64)) == step).all()
    o = int(ex.table[0]["rec_off"])
    assert (ex.rec[o, 1:].astype(np.int64) == ex.rec[o, :-1].astype(np.int64) + 1).all()  # ADDI x2 reads last call's x2 + 1
    # ... and finds the timestamp of that call's last touch of x2 (MUL's second read)
    assert (ex.rec[o + 3, 1:] == ex.rec[0, :-1] + int(ex.table[6]["ts_delta"]) + 1).all()
    # memory written by one call is loaded by the next
    load, store = int(ex.table[1]["rec_off"]), int(ex.table[3]["rec_off"])
    assert (ex.rec[load + 4, 1:] == ex.rec[0, :-1] + int(ex.table[3]["ts_delta"]) + 2).all()
    assert len(ex.initial) == len(ex.final) and 2 in {k[0] for k in ex.initial} and 1 in {k[0] for k in ex.initial}


def test_both_references_agree(closed):
    """ground truth of the executor == what the senders' unbalanced tuples say"""
    got = ref.from_leftovers(bm.tally(closed["senders"])[0], closed["table"])
    for name, t in zip(("program", "connector", "boundary"), got):
        assert (t == closed["traces"][name]).all(), name


def test_constraints_vanish_and_all_six_buses_balance(closed):
    a, tr = closed["airs"], closed["traces"]
    assert ref.eval_constraints(a["boundary"], tr["boundary"]) == []
    assert len(a["program"].cons[1]) == 0 and len(a["connector"].cons[1]) == 0 and len(a["boundary"].cons[1]) == 8
    assert int(tr["boundary"][0].sum()) == len(closed["ex"].initial) and tr["boundary"].shape[1] > len(closed["ex"].initial)  # padding rows exist
    # without the system AIRs the three buses are open (what the suite had so far) ...
    before = unbalanced(closed["senders"])
    assert all(before[b] for b in (0, 1, 2))
    # ... with them every bus is balanced, tuple by tuple
    after = unbalanced(segment(closed))
    assert sorted(after) == list(ALL_BUSES) and all(after[b] == [] for b in ALL_BUSES), {b: v[:2] for b, v in after.items()}


def test_degrees_stay_within_the_bound(closed):
    """Plonky3's rule: a column of either row 1, is_transition 0; the bound is 3"""
    from powdr_amd import prover

    air = closed["airs"]["boundary"]
    rows = prover.row_operands(air.width)
    bc, spans = air.cons
    degs = []
    for off, ln in np.asarray(spans).tolist():
        st, code, ip = [], bc[off:off + ln].tolist(), 0
        while ip < len(code):
            op = code[ip]
            if op == 0:
                st.append(0 if code[ip + 1] == rows.is_transition else 1)
                ip += 2
            elif op == 1:
                st.append(0)
                ip += 2
            elif op == 5:
                ip += 1
            else:
                y, x = st.pop(), st.pop()
                st.append(x + y if op == 4 else max(x, y))
                ip += 1
        degs.append(st[0])
    assert max(degs) == 3 and degs[-1] == 3


def names(air, bad):
    from powdr_amd import system_airs as sa

    return [sa.BOUNDARY_CONSTRAINTS[k][0] for k, _ in bad]


def test_a_duplicated_address_breaks_the_pointer_gap(closed):
    air, t = closed["airs"]["boundary"], closed["traces"]["boundary"].copy()
    n = int(t[0].sum())
    r = next(r for r in range(n - 1) if t[15, r] == 1)
    t[:, r + 1] = t[:, r]  # the same (as, ptr) on two rows, however the gap limbs are chosen ...
    assert "pointer gap" in names(air, ref.eval_constraints(air, t))
    t[16, r], t[17, r] = (P - 1) & 0x1FFFF, 0  # ... even d = -1 written as limbs: the limbs are not the field element
    assert "pointer gap" in names(air, ref.eval_constraints(air, t))


def test_a_valid_row_after_an_invalid_one_breaks_the_order(closed):
    air, t = closed["airs"]["boundary"], closed["traces"]["boundary"].copy()
    n = int(t[0].sum())
    assert n + 1 < t.shape[1]
    t[:, n + 1] = t[:, n - 1]
    bad = dict(zip(names(air, ref.eval_constraints(air, t)), ref.eval_constraints(air, t)))
    assert bad["valid rows first"][1] == [n]  # (the all-zero row n in between also fails to lead into address space as + 1)
    assert set(bad) == {"valid rows first", "next address space"}


def test_a_gap_limb_of_2_to_the_12_leaves_the_range_bus_unbalanced(closed):
    """d_hi = 2^12 with the pointer moved to match satisfies every constraint: only the range check refuses it"""
    air, t = closed["airs"]["boundary"], closed["traces"]["boundary"].copy()
    n = int(t[0].sum())
    r = next(r for r in range(n - 1) if t[15, r] == 1 and t[1, r] == 2 and (r + 2 >= n or t[15, r + 1] == 0))
    t[17, r] = 1 << 12
    t[2, r + 1] = int(t[2, r]) + 1 + int(t[16, r]) + (1 << 29)
    t[3, r + 1], t[4, r + 1] = int(t[2, r + 1]) & 0x1FFFF, int(t[2, r + 1]) >> 17
    assert ref.eval_constraints(air, t) == []
    open_airs = closed["senders"] + [(t, air.inter)]
    with pytest.raises(AssertionError):  # no row of the range checker holds (2^12, 12)
        ref.periphery_airs(bm.tally(open_airs)[0])
    # received by the honest periphery (made for the honest trace) the tuple is left over on bus 3
    honest = segment(closed)
    honest[len(closed["senders"]) + 2] = (t, air.inter)
    left = unbalanced(honest)
    assert (1 << 12, 12) in left[3] and left[0] == [] and left[2] == []


def test_a_wrong_freq_leaves_the_pc_bus_unbalanced(closed):
    freq = closed["traces"]["program"].copy()
    freq[0, 3] += 1
    left = unbalanced(segment(closed, dict(program=freq)))
    assert left[2] == [tuple(closed["table"][:, 3].tolist())] and all(left[b] == [] for b in ALL_BUSES if b != 2)
    freq[0, 3] -= 1
    freq[0, 12] = 1  # a padding row: freq = 0 there
    assert unbalanced(segment(closed, dict(program=freq)))[2] == [tuple(closed["table"][:, 12].tolist())]


def test_rust_binds_the_new_entries():
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name in ("pw_program_frequencies", "pw_memory_boundary_trace", "pw_system_traces_scratch_bytes", "pw_system_traces_peak_bytes",
                 "pw_system_traces_last_stats", "pw_memory_boundary_set_start_slots"):
        assert name in c and r.get(name) == c[name]
