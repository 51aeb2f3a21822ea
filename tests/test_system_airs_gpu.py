"""Device-side traces of the system AIRs (pw_program_frequencies, pw_memory_boundary_trace) against the numpy
references of tests/_system_airs_ref.py, on both expression paths, and the closed segment: instruction AIRs from a chained execution
(tests/_chained_vm.py), the three periphery AIRs in the preprocessed layout and the three system AIRs — every bus balanced, every
constraint satisfied, one proof whose bus sums cancel over all six buses. Every comparison is exact.

The issue asks for memory logs "with a forced tiny table_bytes so the table grows at least twice": table_bytes is an upper bound and
cannot make a table start smaller, so the growth is forced with pw_memory_boundary_set_start_slots (a first table of 64 slots),
and table_bytes is set to the tightest bound that still holds the log."""
import numpy as np
import pytest

from oracle import apc_model as om
from tests import _bus_multiset as bm
from tests import _chained_vm as vm
from tests import _system_airs_ref as ref
from tests.test_bus_check_gpu import BOTH_PATHS, NO_CONS, Segment, check_paths, from_dev, plain_column_uses, set_path, to_dev

pytestmark = pytest.mark.gpu
P = om.P
NQ = 4


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


@pytest.fixture(scope="module")
def execution():
    return vm.Execution(256, seed=7)


def centred(m):
    m = np.asarray(m, np.int64)
    return np.where(m > P // 2, m - P, m)


# ---- the program AIR's multiplicities -------------------------------------------------------------------------------------------------
def fetch_log(log_table, log_rows, seed):
    """a random program of 2^log_table rows and a sender AIR of 2^log_rows rows, [the nine tuple words, mult]: every row fetches a
    random table row `mult` times (0, 1, 2 or -1) -> (program [9, rows], sender cols [10, rows], interactions, the table row per row)"""
    from powdr_amd import periphery

    rng = np.random.default_rng([seed, log_table])
    rows = 1 << log_table
    table = rng.integers(0, P, size=(9, rows)).astype(np.uint32)
    table[0] = 0x1000 + 8 * np.arange(rows)  # pc_base 0x1000, pc_step 8
    pick = rng.integers(0, rows, size=1 << log_rows)
    pick[: 1 << (log_rows - 1)] = pick[: 1 << (log_rows - 1)] % 24  # half of the rows sit in a loop body of 24 instructions
    mult = rng.choice(np.array([0, 1, 1, 1, 2, P - 1], np.int64), size=1 << log_rows)
    cols = np.concatenate([table[:, pick], mult[None].astype(np.uint32)])
    col = periphery._col
    return table, cols, periphery._tables(2, [(col(9), [col(j) for j in range(9)])]), pick


def want_freq(pick, mult, rows):
    return (np.bincount(pick, weights=centred(mult).astype(np.float64), minlength=rows).astype(np.int64) % P).astype(np.uint32)


@BOTH_PATHS
@pytest.mark.parametrize("log_table", [4, 16])
def test_program_frequencies_equal_bincount(gpu, monkeypatch, interpret, log_table):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    set_path(monkeypatch, interpret)
    table, cols, it, pick = fetch_log(log_table, 17, seed=3)
    s = Segment(gpu, [(cols, it)])
    check_paths(s.provers, interpret)
    d_table = to_dev(torch, table)
    freq, n_foreign, first = sa.program_frequencies(s.seg, d_table, log_table, 0x1000, 8)
    want = want_freq(pick, cols[9], 1 << log_table)
    assert n_foreign == 0 and first is None
    assert (from_dev(freq) == want).all()
    again, _, _ = sa.program_frequencies(s.seg, d_table, log_table, 0x1000, 8)
    assert torch.equal(freq, again)  # integer sums: the same bytes whatever the order of arrival
    # = what the tally says the program AIR must receive: with it the PC lookup balances
    air = sa.program_air(table)
    p = air.make_prover(NQ)
    summaries, tuples = prover.check_segment_buses(s.seg + [(p, freq.data_ptr(), log_table)], buses=[2], tally_all=True)
    assert summaries[0]["status"] == 0 and summaries[0]["n_active"] > 1 << 16 and tuples == []
    p.close()
    s.close()


@BOTH_PATHS
def test_foreign_instructions_are_counted_and_named(gpu, monkeypatch, interpret):
    torch, prover = gpu
    from powdr_amd import periphery
    from powdr_amd import system_airs as sa

    set_path(monkeypatch, interpret)
    table, cols, it, pick = fetch_log(4, 10, seed=5)
    cols = cols.copy()
    cols[9] = 1
    honest = want_freq(pick, cols[9], 16)
    bad = {40: (0, 0x1000 + 8 * 16), 41: (0, 0x1000 - 8), 77: (0, 0x1000 + 8 * 3 + 4), 300: (5, (int(cols[5, 300]) + 1) % P)}  # row: (column, value)
    for r, (c, v) in bad.items():  # past the table, below pc_base, misaligned, one word different
        cols[c, r] = v
    good = np.ones(1 << 10, bool)
    good[list(bad)] = False
    # a second AIR on the same bus whose tuples have eight words: every one of its active rows is foreign
    col = periphery._col
    short = (cols[:9, :8].copy(), periphery._tables(2, [(col(8), [col(j) for j in range(8)])]))
    short[0][8] = (1, 0, 1, 1, 0, 0, 0, 0)
    s = Segment(gpu, [(cols, it), short])
    d_table = to_dev(torch, table)
    freq, n_foreign, first = sa.program_frequencies(s.seg, d_table, 4, 0x1000, 8)
    assert n_foreign == len(bad) + 3
    assert first == dict(bus=2, n_args=9, args=cols[:9, 40].tolist(), net_multiplicity=1, air=0, interaction=0, row=40, n_contributions=1)
    want = want_freq(pick[good], cols[9][good], 16)
    assert (from_dev(freq) == want).all() and (want != honest).any()  # freq is what the honest rows alone give
    # only the short AIR foreign: its first active row is named, with its eight words
    s2 = Segment(gpu, [short])
    _, n2, first2 = sa.program_frequencies(s2.seg, d_table, 4, 0x1000, 8)
    assert n2 == 3 and (first2["n_args"], first2["args"], first2["row"]) == (8, short[0][:8, 0].tolist(), 0)
    # malformed arguments: -1, nothing touched
    from powdr_amd import abi

    with pytest.raises(abi.HipError):
        sa.program_frequencies(s.seg, d_table, 4, 0x1000, 0)
    s.close()
    s2.close()


# ---- the memory boundary AIR's trace -----------------------------------------------------------------------------------------------
def boundary_of(gpu, seg, want, **kw):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    cap = (want.shape[1] - 1).bit_length()
    trace, lh, locations, status = sa.memory_boundary_trace(seg, cap, **kw)
    assert status == 0 and locations == int(want[0].sum()) and 1 << lh == want.shape[1]
    got = from_dev(trace).reshape(18, 1 << lh)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    return trace


@BOTH_PATHS
@pytest.mark.parametrize("log_rows,locations", [(10, 600), (16, 30000), (20, 400000)])
def test_memory_logs_equal_the_reference_word_for_word(gpu, monkeypatch, interpret, log_rows, locations):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    set_path(monkeypatch, interpret)
    cols, want = ref.memory_log(log_rows, locations, seed=11)
    n = int(want[0].sum())
    s = Segment(gpu, [(cols, ref.memory_log_interactions())])
    check_paths(s.provers, interpret)
    slots = 64
    while slots - slots // 8 < n:  # a table is full at 7/8: the smallest power of two that holds the log is the bound
        slots *= 4
    sa.set_boundary_start_slots(6)
    try:
        a = boundary_of(gpu, s.seg, want, table_bytes=40 * slots)
        stats = sa.last_stats()
        assert stats["tables"] >= 3 and stats["occupied_slots"] == n and stats["table_slots"] <= slots
        b = boundary_of(gpu, s.seg, want, table_bytes=40 * slots)
        assert torch.equal(a, b)
    finally:
        sa.set_boundary_start_slots(0)
    c = boundary_of(gpu, s.seg, want)  # the default table: the same bytes
    assert torch.equal(a, c) and sa.last_stats()["scratch_bytes"] < 64 << 10 < sa.last_stats()["peak_bytes"]
    # the trace closes the log's memory bus, and satisfies the AIR's constraints on the device
    air = sa.boundary_air()
    p = air.make_prover(NQ)
    lh = (want.shape[1] - 1).bit_length()
    assert p.check_constraints(a.data_ptr(), lh) == (0, None, None)
    summaries, tuples = prover.check_segment_buses(s.seg + [(p, a.data_ptr(), lh)], buses=[1])
    assert summaries == [dict(bus=1, status=0, n_active=2 * ((1 << log_rows) - 5) + 2 * n, n_unbalanced=0)] and tuples == []
    p.close()
    s.close()


def test_statuses_one_to_four(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import abi, periphery
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    cols, want = ref.memory_log(10, 600, seed=2)
    n, it = int(want[0].sum()), ref.memory_log_interactions()
    s = Segment(gpu, [(cols, it)])
    # 1: the cap is too small; what is needed comes back and the second call succeeds
    trace, lh, locations, status = sa.memory_boundary_trace(s.seg, 3)
    assert (trace, lh, locations, status) == (None, 10, n, 1)
    trace, lh, locations, status = sa.memory_boundary_trace(s.seg, lh)
    assert status == 0 and (from_dev(trace).reshape(18, -1) == want).all()
    # 2: a table bound of 512 slots holds 448 locations, not 600 — the same answer every time
    for _ in range(2):
        assert sa.memory_boundary_trace(s.seg, 10, table_bytes=40 * 512)[1:] == (0, 0, 2)
        assert sa.last_stats()["scratch_bytes"] < 64 << 10  # (the table that overflowed at the bound is gone again)
    assert sa.memory_boundary_trace(s.seg, 10, table_bytes=39)[3] == 2
    # 3: one row counts twice
    twice = cols.copy()
    twice[12, 17] = 2
    s3 = Segment(gpu, [(twice, it)])
    assert sa.memory_boundary_trace(s3.seg, 10)[3] == 3 and sa.last_stats()["scratch_bytes"] < 64 << 10  # (raised with the table allocated)
    # 4: a location that is only written: a second AIR with the send alone, at an address nobody else touches
    col = periphery._col
    lone = np.zeros((13, 4), np.uint32)
    lone[:, 1] = [2, 0x1FFFFFFC, 0, 0, 0, 0, 0, 1, 2, 3, 4, 5000, 1]
    send_only = periphery._tables(1, [(col(12), [col(0), col(1)] + [col(7 + i) for i in range(4)] + [col(11)])])
    s4 = Segment(gpu, [(cols, it), (lone, send_only)])
    trace, lh, locations, status = sa.memory_boundary_trace(s4.seg, 11)
    assert (trace, locations, status) == (None, n + 1, 4)
    # malformed: a tuple on the bus that is no (as, ptr, 4 words, timestamp); a cap of 0
    six = periphery._tables(1, [(col(12), [col(0), col(1)] + [col(7 + i) for i in range(4)])])
    s5 = Segment(gpu, [(cols, it), (lone, six)])
    with pytest.raises(abi.HipError):
        sa.memory_boundary_trace(s5.seg, 11)
    with pytest.raises(abi.HipError):
        sa.memory_boundary_trace(s.seg, 0)
    for bad in (5, 31):  # the first table has 2^6 .. 2^30 slots
        with pytest.raises(abi.HipError):
            sa.set_boundary_start_slots(bad)
    for x in (s, s3, s4, s5):
        x.close()


# ---- the closed segment -----------------------------------------------------------------------------------------------------------------
class Closed:
    """instruction AIRs of the chained execution on the device, closed by close_segment, with the periphery AIRs in the preprocessed
    layout made AFTER it (their histograms hold the boundary AIR's lookups too)"""

    def __init__(self, gpu, ex, tamper=None):
        torch, prover = gpu
        from powdr_amd import periphery, tracegen
        from powdr_amd import system_airs as sa
        from powdr_amd.segment_workload import BusReplay

        self.per = tracegen.Periphery.fresh()
        self.airs = []
        for name, t, (bc, sp, it) in ex.instruction_airs():
            t = t.copy()
            if tamper is not None:
                tamper(name, t, it)
            lh = t.shape[1].bit_length() - 1
            p = prover.Prover(t.shape[0], bc, sp, num_queries=NQ, interactions=it)
            self.airs.append(dict(name=name, role="instruction", width=t.shape[0], log_h=lh, cons=(bc, sp), inter=it, trace=to_dev(torch, t), prover=p, pre=None))
        torch.cuda.synchronize()
        self.senders = [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in self.airs]
        for a in self.airs:
            BusReplay(a["inter"], 1 << a["log_h"])(a["trace"].data_ptr(), self.per)
        self.airs = sa.close_segment(self.airs, ex.program_table(), ex.start_pc, self.per, num_queries=NQ)
        per = self.per
        for name, hist, it, table, pre_w in (("var_range", per.var_hist, periphery.var_range_interactions_pre(), periphery.var_range_table(per.var_hist.numel()), 2),
                                             ("tuple2", per.tuple_hist, periphery.tuple2_interactions_pre(), periphery.tuple2_table(per.tuple_sizes), 2),
                                             ("bitwise", per.bitwise_hist, periphery.bitwise_interactions_pre(), periphery.bitwise_table(), 3)):
            lh = (hist.numel() // (2 if name == "bitwise" else 1)).bit_length() - 1
            torch.cuda.synchronize()
            pre = (table, pre_w, lh)
            p = prover.Prover(hist.numel() >> lh, *NO_CONS, num_queries=NQ, interactions=it, preprocessed=pre)
            self.airs.append(dict(name=name, role="periphery", width=hist.numel() >> lh, log_h=lh, cons=NO_CONS, inter=it, trace=periphery.multiplicities(hist),
                                  prover=p, pre=pre))
        torch.cuda.synchronize()
        self.seg = [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in self.airs]

    def by_name(self, name):
        return next(a for a in self.airs if a["name"] == name)

    def close(self):
        for a in self.airs:
            a["prover"].close()


@pytest.fixture(scope="module", params=[False, True], ids=["small_forms", "interpreter"])
def closed(gpu, execution, request):
    import os

    old = os.environ.pop("POWDR_LOGUP_INTERPRET", None)
    if request.param:
        os.environ["POWDR_LOGUP_INTERPRET"] = "1"
    try:
        c = Closed(gpu, execution)
    finally:
        os.environ.pop("POWDR_LOGUP_INTERPRET", None)
        if old is not None:
            os.environ["POWDR_LOGUP_INTERPRET"] = old
    check_paths([a["prover"] for a in c.airs], request.param)
    yield c
    c.close()


def test_generated_system_traces_equal_the_reference(gpu, execution, closed):
    ex = execution
    table = ex.program_table()
    want = dict(program=ref.program_freq(table, {ex.start_pc + 4 * i: ex.calls for i in range(len(ex.block))}),
                connector=ref.connector_trace(ex.start, ex.end), boundary=ref.boundary_trace(ex.initial, ex.final))
    for name, w in want.items():
        a = closed.by_name(name)
        assert (from_dev(a["trace"]).reshape(w.shape) == w).all(), name
        assert a["log_h"] == w.shape[1].bit_length() - 1
    # and the reference built from the senders' leftover tuples alone
    host = [(from_dev(a["trace"]).reshape(a["width"], -1), a["inter"]) for a in closed.airs if a["role"] == "instruction"]
    for name, w in zip(("program", "connector", "boundary"), ref.from_leftovers(bm.tally(host)[0], table)):
        assert (w == want[name]).all(), name


def test_the_closed_segment_balances_all_six_buses_and_proves(gpu, closed):
    torch, prover = gpu
    summaries, tuples = prover.check_segment_buses(closed.seg)
    assert [s["bus"] for s in summaries] == [0, 1, 2, 3, 6, 7]
    assert all(s["status"] == 0 and s["n_active"] > 0 and s["n_unbalanced"] == 0 for s in summaries) and tuples == []
    assert prover.check_segment_buses(closed.seg, tally_all=True) == (summaries, tuples)  # the exact tally agrees with the sums
    for a in closed.airs:
        assert a["prover"].check_constraints(a["trace"].data_ptr(), a["log_h"]) == (0, None, None), a["name"]
    assert closed.by_name("boundary")["prover"].row_flags == 3 and closed.by_name("boundary")["prover"].max_constraint_degree() == 3
    proof = prover.prove_segment(closed.seg, logup=True)
    descs = [(a["width"], a["log_h"], a["cons"][0], a["cons"][1], a["inter"]) for a in closed.airs]
    keys = [None if a["pre"] is None else (a["pre"][1], a["prover"].preprocessed_root()) for a in closed.airs]
    rc, total = prover.verify_segment(descs, proof, NQ, 0, True, check_balance=True, preprocessed=keys, transition=True)
    assert rc == 0 and not np.asarray(total).any()
    # without the three system AIRs the same statement does not balance (what every segment proof here was so far)
    keep = [i for i, a in enumerate(closed.airs) if a["role"] != "system"]
    open_proof = prover.prove_segment([closed.seg[i] for i in keep], logup=True)
    rc, total = prover.verify_segment([descs[i] for i in keep], open_proof, NQ, 0, True, check_balance=True, preprocessed=[keys[i] for i in keep],
                                      transition=True)
    assert rc == 14 and np.asarray(total).any()


def test_generation_leaves_the_callers_traces_and_proofs_alone(gpu, closed):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    senders = [a for a in closed.airs if a["role"] == "instruction"]
    seg = [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in senders]
    before = [a["trace"].clone() for a in senders]
    p1 = prover.prove_segment(seg, logup=True)
    prog = closed.by_name("program")
    freq, n_foreign, _ = sa.program_frequencies(seg, prog["pre"][0], prog["log_h"], vm.START_PC)
    trace, lh, _, status = sa.memory_boundary_trace(seg, 12)
    con = sa.connector_trace(seg)
    torch.cuda.synchronize()
    assert n_foreign == 0 and status == 0
    assert torch.equal(freq, prog["trace"]) and torch.equal(trace, closed.by_name("boundary")["trace"]) and torch.equal(con, closed.by_name("connector")["trace"])
    assert all(torch.equal(x, a["trace"]) for x, a in zip(before, senders))
    p2 = prover.prove_segment(seg, logup=True)
    assert len(p1) == len(p2) and (p1 == p2).all()
    assert sa.last_stats()["scratch_bytes"] < 64 << 10


def test_a_changed_stored_word_leaves_the_memory_bus_unbalanced_and_is_named(gpu, execution, monkeypatch):
    """One byte of the word call 100 stores is changed in the LoadStore trace. The boundary trace is still made (status 0: the routine
    pairs first receives with last sends and proves nothing); the bus check on bus 1 then names the two tuples of the broken link: the
    changed send and the receive of call 101's load, which still expects the honest word."""
    torch, prover = gpu
    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex = execution
    store = ex.table[3]
    call = 100
    found = {}

    def tamper(name, t, it):
        if name != "LoadStore":
            return
        row = int(store["air_row"]) + call * ex.rbs[int(store["kind"])]
        plain, uses = plain_column_uses(it)
        inter = np.asarray(it[0]).reshape(-1, 3)
        host = [(t[:, row:row + 1], it)]
        sends = {k[2]: e for k, e in bm.tally(host)[0].items() if k[0] == 1 and e[0] == 1 and k[2][0] == 2}  # the store's write to memory
        assert len(sends) == 1
        (args, (_, (_, i, _), _)), = sends.items()
        c = next(c for c, where in sorted(plain.items()) if where == [(i, 2)] and uses[c] == 1)  # the column of its first data byte
        assert int(inter[i, 0]) == 1 and int(t[c, row]) == args[2]
        t[c, row] = (int(t[c, row]) + 1) % 256
        moved = list(args)
        moved[2] = int(t[c, row])
        found.update(honest=list(args), moved=moved, row=row, inter=i)

    c = Closed(gpu, ex, tamper)
    air = next(k for k, a in enumerate(c.airs) if a["name"] == "LoadStore")
    summaries, tuples = prover.check_segment_buses(c.seg, buses=[0, 1, 2])
    assert [s["status"] for s in summaries] == [0, 1, 0] and summaries[1]["n_unbalanced"] == 2
    assert sorted((t["args"], t["net_multiplicity"]) for t in tuples) == sorted([(found["honest"], P - 1), (found["moved"], 1)])
    sent = next(t for t in tuples if t["net_multiplicity"] == 1)
    assert (sent["air"], sent["interaction"], sent["row"]) == (air, found["inter"], found["row"])
    lost = next(t for t in tuples if t["net_multiplicity"] == P - 1)
    assert lost["air"] == air and lost["row"] == int(ex.table[1]["air_row"]) + (call + 1) * ex.rbs[int(store["kind"])]
    c.close()
