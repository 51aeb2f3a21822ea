"""pw_check_segment_buses on the GPU against the numpy multiset of tests/_bus_multiset.py: summaries, tuples, net
multiplicities, witnesses and contribution counts, on both expression paths (small forms; POWDR_LOGUP_INTERPRET=1: the interpreter)."""
import numpy as np
import pytest

from oracle import apc_model as om
from tests import _bus_multiset as bm

pytestmark = pytest.mark.gpu
P = om.P
BOTH_PATHS = pytest.mark.parametrize("interpret", [False, True], ids=["small_forms", "interpreter"])
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def to_dev(torch, canonical):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(canonical, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()


def from_dev(t):
    return om.from_monty(t.cpu().numpy().view(np.uint32))


def set_path(monkeypatch, interpret):
    if interpret:
        monkeypatch.setenv("POWDR_LOGUP_INTERPRET", "1")
    else:
        monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)


def check_paths(provers, interpret):
    paths = [p.logup_path() for p in provers]
    assert all(x == 1 for x in paths) if interpret else 2 in paths, paths


class Segment:
    """host AIRs [(cols [columns, rows] canonical, interactions)] on the device, one plain LogUp prover each"""

    def __init__(self, gpu, host):
        torch, prover = gpu
        self.host = host
        self.provers = [prover.Prover(len(cols), *NO_CONS, num_queries=2, interactions=it) for cols, it in host]
        self.traces = [to_dev(torch, cols) for cols, _ in host]
        self.seg = [(p, t.data_ptr(), len(cols[0]).bit_length() - 1) for p, t, (cols, _) in zip(self.provers, self.traces, host)]

    def close(self):
        for p in self.provers:
            p.close()


def compare(prover, seg, host, buses=None, tally_all=False, cap=1 << 16, **kw):
    summaries, tuples = prover.check_segment_buses(seg, buses=buses, tally_all=tally_all, tuple_cap=cap, **kw)
    want_s, want_t = bm.expected(host, buses, tally_all)
    assert summaries == want_s
    assert len(tuples) == min(cap, len(want_t))
    for got, want in zip(tuples, want_t):
        assert got == want
    return summaries, tuples


# ---- 1 - 4: random AIRs ------------------------------------------------------------------------------------------------------------
RANDOM_SPEC = [("T0", 5), ("T1", 200), ("T1", 3000), ("T0", 30)]  # heights 2^3, 2^8, 2^12, 2^5


def random_airs():
    """the interaction tables of synthetic APCs over random traces with cells in {0, 1}: the tuples repeat, so that the tally has sums
    to form, and about a thousand of them do not cancel"""
    from tests.test_segment_proof import synthetic_airs

    rng = np.random.default_rng(5)
    return [(rng.integers(0, 2, size=(a[1], 1 << a[2])).astype(np.uint32), a[5]) for a in synthetic_airs(RANDOM_SPEC, seed0=21)]


@pytest.fixture(scope="module")
def random_host():
    host = random_airs()
    want_s, want_t = bm.expected(host, None, True)
    assert len(want_s) == 5 and all(s["status"] == 1 for s in want_s)
    assert 300 <= len(want_t) <= 3000  # (a CPU-side property of the inputs: enough unbalanced tuples to order, few enough to list)
    assert {len(c[0]) for c, _ in host} == {8, 256, 4096, 32}
    return host


@BOTH_PATHS
def test_random_airs_equal_the_numpy_multiset(gpu, random_host, monkeypatch, interpret):
    torch, prover = gpu
    set_path(monkeypatch, interpret)
    s = Segment(gpu, random_host)
    check_paths(s.provers, interpret)
    summaries, tuples = compare(prover, s.seg, random_host, tally_all=True)
    assert sum(x["n_unbalanced"] for x in summaries) == len(tuples) >= 300
    # a subset of the buses, and a bus nobody uses
    compare(prover, s.seg, random_host, buses=[6, 3, 3, 99], tally_all=True)
    # without tally_all: the same (every bus is unbalanced here, so every bus is tallied)
    compare(prover, s.seg, random_host)
    # seed independence: everything reported is the same
    a = prover.check_segment_buses(s.seg, seed=1, tally_all=True, tuple_cap=1 << 16)
    b = prover.check_segment_buses(s.seg, seed=0xDEADBEEFCAFE, tally_all=True, tuple_cap=1 << 16)
    assert a == b == (summaries, tuples)
    # truncation: the lexicographically first tuple, the full count
    s1, t1 = prover.check_segment_buses(s.seg, tally_all=True, tuple_cap=1)
    assert s1 == summaries and t1 == tuples[:1]
    s0, t0 = prover.check_segment_buses(s.seg, tuple_cap=0)
    assert s0 == summaries and t0 == []
    s.close()


@BOTH_PATHS
def test_a_table_too_small_gives_status_2_for_that_bus_only(gpu, random_host, monkeypatch, interpret):
    torch, prover = gpu
    set_path(monkeypatch, interpret)
    s = Segment(gpu, random_host)
    table, _ = bm.tally(random_host)
    distinct = {}
    for bus, _, _ in table:
        distinct[bus] = distinct.get(bus, 0) + 1
    slots = 16
    holds = slots - slots // 8  # documented: a table counts as full at 7/8 of its slots
    assert any(n > holds for n in distinct.values()) and any(n <= holds for n in distinct.values())
    want_s, want_t = bm.expected(random_host, None, True)
    for x in want_s:
        if distinct[x["bus"]] > holds:
            x.update(status=2, n_unbalanced=0)
    want_t = [t for t in want_t if distinct[t["bus"]] <= holds]
    for _ in range(2):  # (the status for a given table_bytes is deterministic)
        got_s, got_t = prover.check_segment_buses(s.seg, table_bytes=40 * slots + 39, tally_all=True, tuple_cap=1 << 16)  # rc 0: no exception
        assert got_s == want_s and got_t == want_t
    # not even one slot
    got_s, got_t = prover.check_segment_buses(s.seg, table_bytes=39)
    assert [x["status"] for x in got_s] == [2] * 5 and got_t == []
    s.close()


@BOTH_PATHS
def test_the_table_grows_until_it_holds_the_bus(gpu, monkeypatch, interpret):
    """A bus of 2^18 distinct tuples sent once and never received: more than the first table of 2^16 slots and more than 7/8 of the
    next one of 2^18, so the default (and a bound of 2^20 slots) names them from the third table — 2^19 slots, twice the active triples:
    no bus gets more — a bound of 2^18 slots gives status 2, every time, and the peak scratch is that table of 20 MiB plus 28 bytes per
    listed tuple (7 MiB), whatever room the device has."""
    torch, prover = gpu
    set_path(monkeypatch, interpret)
    H = 1 << 18
    from tests.test_preprocessed_segment_gpu import PA, tables

    host = [(np.stack([np.arange(H, dtype=np.uint32), np.ones(H, np.uint32)]), tables([(11, [PA, 1], [[PA, 0]])]))]  # sends (row) once
    assert bm.expected(host, None, True)[0] == [dict(bus=11, status=1, n_active=H, n_unbalanced=H)]
    s = Segment(gpu, host)
    first = [dict(bus=11, n_args=1, args=[k], net_multiplicity=1, air=0, interaction=0, row=k, n_contributions=1) for k in range(3)]
    for kw in (dict(), dict(table_bytes=40 << 20)):
        for _ in range(2):
            got_s, got_t = prover.check_segment_buses(s.seg, tuple_cap=3, **kw)
            assert got_s == [dict(bus=11, status=1, n_active=H, n_unbalanced=H)] and got_t == first
            assert 20 << 20 <= prover.bus_check_peak_bytes() <= 28 << 20
    for _ in range(2):
        got_s, got_t = prover.check_segment_buses(s.seg, tuple_cap=3, table_bytes=40 << 18)
        assert got_s == [dict(bus=11, status=2, n_active=H, n_unbalanced=0)] and got_t == []
        assert prover.bus_check_scratch_bytes() <= 64 << 10  # (the table that overflowed at the bound is gone again)
    s.close()


# ---- 9: arity, and sums that reach exactly p ----------------------------------------------------------------------------------------
@BOTH_PATHS
def test_a_pair_and_a_triple_with_a_zero_are_different_tuples(gpu, monkeypatch, interpret):
    torch, prover = gpu
    from tests.test_bus_check_cpu import hand_example

    set_path(monkeypatch, interpret)
    (a0, it0), (a1, it1) = hand_example()
    host = [(np.concatenate([a0, np.zeros((a0.shape[0], 2), np.int64)], axis=1), it0), (a1, it1)]  # 8 and 4 rows
    s = Segment(gpu, host)
    summaries, tuples = compare(prover, s.seg, host, tally_all=True)
    assert [(t["n_args"], t["args"]) for t in tuples] == [(2, [0, 0]), (2, [7, 8]), (3, [7, 8, 0])]
    assert summaries[1] == dict(bus=9, status=0, n_active=4, n_unbalanced=0)  # (p + 1) / 2 + (p - 1) / 2
    # (a proof's LogUp sum would cancel (7, 8) sent three times against (7, 8, 0) received three times: DESIGN.md §5i)
    s.close()


# ---- 8: the forged var-range row ----------------------------------------------------------------------------------------------------
@BOTH_PATHS
def test_the_forged_range_check(gpu, monkeypatch, interpret):
    torch, prover = gpu
    from powdr_amd import abi, periphery
    from tests.test_preprocessed_segment_gpu import BINS_LOG, SEND, sender_trace

    set_path(monkeypatch, interpret)
    nb = 1 << BINS_LOG
    snd = prover.Prover(3, *NO_CONS, num_queries=4, interactions=SEND)
    forged = to_dev(torch, sender_trace(300, 8))
    # main layout: the receiver's tuple columns are the prover's to fill — the forged row balances the send, as that layout means
    recv_t = om.var_range_trace(np.zeros(nb, np.uint32))
    recv_t[:, 0] = (300, 8, 1)
    rcv = prover.Prover(3, *NO_CONS, num_queries=4, interactions=periphery.var_range_interactions())
    recv_d = to_dev(torch, recv_t)
    summaries, tuples = prover.check_segment_buses([(snd, forged.data_ptr(), 2), (rcv, recv_d.data_ptr(), BINS_LOG)], tally_all=True)
    assert summaries == [dict(bus=3, status=0, n_active=2, n_unbalanced=0)] and tuples == []
    # preprocessed layout: the table is the key's; (300, 8) is in no row of it
    table = periphery.var_range_table(nb)
    pre = prover.Prover(1, *NO_CONS, num_queries=4, interactions=periphery.var_range_interactions_pre(), preprocessed=(table, 2, BINS_LOG))
    mult_t = to_dev(torch, np.zeros(nb, np.uint32))
    for tally_all in (False, True):
        summaries, tuples = prover.check_segment_buses([(snd, forged.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)], tally_all=tally_all)
        assert summaries == [dict(bus=3, status=1, n_active=1, n_unbalanced=1)]
        assert tuples == [dict(bus=3, n_args=2, args=[300, 8], net_multiplicity=1, air=0, interaction=0, row=0, n_contributions=1)]
    # an honest send with its multiplicity: balanced; the receive then names the table's row
    honest = to_dev(torch, sender_trace(200, 8))
    mult = np.zeros(nb, np.uint32)
    mult[(1 << 8) + 200 - 1] = 1
    mult_t = to_dev(torch, mult)
    summaries, tuples = prover.check_segment_buses([(snd, honest.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)], tally_all=True)
    assert summaries == [dict(bus=3, status=0, n_active=2, n_unbalanced=0)] and tuples == []
    summaries, tuples = prover.check_segment_buses([(snd, forged.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)])
    assert [(t["args"], t["net_multiplicity"], t["air"], t["row"]) for t in tuples] == [([200, 8], P - 1, 1, (1 << 8) + 200 - 1), ([300, 8], 1, 0, 0)]
    # a preprocessed prover at another height than its own: -1; and one that occurs twice (its staging matrix holds one trace)
    with pytest.raises(abi.HipError):
        prover.check_segment_buses([(pre, mult_t.data_ptr(), BINS_LOG - 1)])
    with pytest.raises(abi.HipError):
        prover.check_segment_buses([(pre, mult_t.data_ptr(), BINS_LOG), (snd, forged.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)])
    # a prover made without interaction tables contributes nothing
    bare = prover.Prover(3, *NO_CONS, num_queries=4)
    assert prover.check_segment_buses([(bare, forged.data_ptr(), 2)]) == ([], [])
    assert prover.check_segment_buses([(bare, forged.data_ptr(), 2), (snd, forged.data_ptr(), 2)], buses=[3])[0][0]["n_active"] == 1
    for p in (snd, rcv, pre, bare):
        p.close()


# ---- 5 - 7, 10: the honest segment ---------------------------------------------------------------------------------------------------
def host_airs(seg):
    out = []
    for a in seg.airs:
        W, H = a["width"], 1 << a["log_h"]
        cols = from_dev(a["trace"][:W * H]).reshape(W, H)
        if a.get("pre") is not None:
            t, pre_w, _ = a["pre"]
            cols = np.concatenate([cols, from_dev(t).reshape(pre_w, H)])
        out.append((cols, a["inter"]))
    return out


def bump_cell(t, index, delta):
    """one Montgomery cell of a device trace += delta (canonical)"""
    v = int(om.from_monty(np.array([t[index].item()], np.int32).view(np.uint32))[0])
    t[index] = int(om.to_monty(np.array([(v + delta) % P], np.uint32)).view(np.int32)[0])


def plain_column_uses(interactions):
    """{column: [(interaction, argument)]} for arguments that are exactly one column, and the set of columns the table reads at all"""
    inter, spans, bc = (np.asarray(x) for x in interactions)
    plain, count = {}, {}
    for i, (_, n_args, first) in enumerate(inter.reshape(-1, 3).tolist()):
        for k in range(n_args + 1):
            off, ln = spans.reshape(-1, 2)[first + k]
            code, ip = bc[off:off + ln].tolist(), 0
            while ip < len(code):
                if code[ip] in (0, 1):
                    if code[ip] == 0:
                        count[code[ip + 1]] = count.get(code[ip + 1], 0) + 1
                    ip += 1
                ip += 1
            if k and code[0] == 0 and len(code) == 2:
                plain.setdefault(code[1], []).append((i, k - 1))
    return plain, count


@pytest.fixture(scope="module", params=[("main", False), ("main", True), ("preprocessed", False), ("preprocessed", True)],
                ids=["main-small_forms", "main-interpreter", "preprocessed-small_forms", "preprocessed-interpreter"])
def honest(gpu, request):
    import os
    from powdr_amd import segment_workload as sw

    layout, interpret = request.param
    old = os.environ.pop("POWDR_LOGUP_INTERPRET", None)
    if interpret:
        os.environ["POWDR_LOGUP_INTERPRET"] = "1"
    try:
        seg = sw.HonestSegment("C4", max_log_height=9, seed=2, queries=4, pow_bits=0, logup=True, max_apc_airs=2, periphery_layout=layout)
    finally:
        os.environ.pop("POWDR_LOGUP_INTERPRET", None)
        if old is not None:
            os.environ["POWDR_LOGUP_INTERPRET"] = old
    check_paths([a["prover"] for a in seg.airs], interpret)
    yield seg
    seg.close()


def test_honest_segment_lookup_buses_balance_and_send_only_buses_do_not(gpu, honest):
    torch, prover = gpu
    from powdr_amd import synth
    from powdr_amd.segment_workload import LOOKUP_BUSES

    seg = honest
    seg.generate_traces()
    torch.cuda.synchronize()
    host = host_airs(seg)
    summaries, tuples = seg.check_buses()
    assert [s["bus"] for s in summaries] == sorted(LOOKUP_BUSES)
    assert all(s["status"] == 0 and s["n_active"] > 0 and s["n_unbalanced"] == 0 for s in summaries) and tuples == []
    assert (summaries, tuples) == bm.expected(host, LOOKUP_BUSES)
    assert (summaries, tuples) == seg.check_buses(LOOKUP_BUSES, tally_all=True)  # the exact pass agrees with the sums
    rc, total = seg.balance_witness()
    assert rc == 0 and not np.asarray(total).any()
    # every bus: the lookup buses as before; memory, execution bridge and pc lookup have only senders here
    cap = 1 << 15
    summaries, tuples = seg.check_buses(None, tuple_cap=cap)
    want_s, want_t = bm.expected(host, None)
    assert summaries == want_s and tuples == want_t[:cap]
    by_bus = {s["bus"]: s for s in summaries}
    assert all(by_bus[b]["status"] == 0 for b in LOOKUP_BUSES)
    for b in (synth.BUS_MEMORY, synth.BUS_EXEC, synth.BUS_PC):
        assert by_bus[b]["status"] == 1 and by_bus[b]["n_active"] > 0 and by_bus[b]["n_unbalanced"] > 0


def test_tampered_cells_are_named(gpu, honest):
    torch, prover = gpu
    from powdr_amd import synth

    seg = honest
    seg.generate_traces()
    torch.cuda.synchronize()
    host = host_airs(seg)
    table, _ = bm.tally(host)
    # a var-range tuple with ONE sender, in an APC AIR, whose value is a plain column that no other span of that AIR reads
    found = None
    for (bus, n_args, args), (net, (air, inter, row), count) in sorted(table.items()):
        if bus != synth.BUS_VAR_RANGE or count != 2 or net or seg.airs[air]["role"] != "apc":
            continue
        plain, uses = plain_column_uses(seg.airs[air]["inter"])
        cols = [c for c, where in plain.items() if where == [(inter, 0)] and uses[c] == 1]
        if cols:
            found = (air, inter, row, cols[0], args)
            break
    assert found is not None, "no singly-sent var-range tuple in this segment (a property of the inputs)"
    air, inter, row, col, args = found
    a = seg.airs[air]
    index = col * (1 << a["log_h"]) + row
    delta = 1 << 24  # a value no range check of at most 2^17 bins receives and nobody else sends
    assert (synth.BUS_VAR_RANGE, 2, (args[0] + delta, args[1])) not in table
    bump_cell(a["trace"], index, delta)
    torch.cuda.synchronize()
    summaries, tuples = seg.check_buses()
    assert [s["status"] for s in summaries] == [1, 0, 0] and summaries[0]["n_unbalanced"] == 2
    per_air = [k for k, x in enumerate(seg.airs) if x["name"] == "var_range"][0]
    assert len(tuples) == 2
    lost, extra = tuples  # ordered by the value: the honest one first
    assert (lost["args"], lost["net_multiplicity"], lost["air"], lost["n_contributions"]) == (list(args), P - 1, per_air, 1)
    assert extra == dict(bus=synth.BUS_VAR_RANGE, n_args=2, args=[args[0] + delta, args[1]], net_multiplicity=1, air=air, interaction=inter,
                         row=row, n_contributions=1)
    assert (summaries, tuples) == bm.expected(host_airs(seg), (3, 6, 7))
    assert seg.balance_witness()[0] == 14
    bump_cell(a["trace"], index, P - delta)
    torch.cuda.synchronize()
    assert seg.check_buses()[1] == []
    # one periphery multiplicity too many: exactly one tuple, received once more than it was sent
    per = seg.airs[per_air]
    H = 1 << per["log_h"]
    mult_col = 0 if per.get("pre") is not None else 2
    t_row = int(np.nonzero(host[per_air][0][mult_col])[0][0])  # a row whose tuple was sent (and received as often)
    bump_cell(per["trace"], mult_col * H + t_row, 1)
    torch.cuda.synchronize()
    summaries, tuples = seg.check_buses()
    assert summaries[0]["status"] == 1 and summaries[0]["n_unbalanced"] == 1 and len(tuples) == 1
    assert tuples[0]["net_multiplicity"] == P - 1 and tuples[0]["air"] < per_air  # (its sender is the smaller witness)
    assert (summaries, tuples) == bm.expected(host_airs(seg), (3, 6, 7))
    assert seg.balance_witness()[0] == 14
    bump_cell(per["trace"], mult_col * H + t_row, P - 1)
    torch.cuda.synchronize()
    assert seg.check_buses()[1] == []


def test_the_check_leaves_proofs_traces_and_memory_alone(gpu, honest):
    torch, prover = gpu
    seg = honest
    seg.generate_traces()
    p1 = seg.prove(copy=True)
    torch.cuda.synchronize()
    before = [a["trace"].clone() for a in seg.airs]
    held = seg.device_bytes() + prover.segment_context_bytes()
    summaries, _ = seg.check_buses(None, tally_all=True, tuple_cap=16)
    assert any(s["status"] == 1 for s in summaries)
    scratch = prover.bus_check_scratch_bytes()
    orders = sum(4 * len(np.asarray(a["inter"][0]).reshape(-1, 3)) for a in seg.airs)
    # documented: 4 bytes per interaction in every prover, a few kilobytes of per-thread tables; the tally table is gone again
    assert scratch <= 64 << 10 and prover.bus_check_peak_bytes() > scratch
    assert seg.device_bytes() + prover.segment_context_bytes() <= held + orders
    torch.cuda.synchronize()
    assert all(torch.equal(x, a["trace"]) for x, a in zip(before, seg.airs))
    p2 = seg.prove(copy=True)
    assert len(p1) == len(p2) and (p1 == p2).all() and seg.verify(p2) == 0
    assert seg.device_bytes() + prover.segment_context_bytes() <= held + orders


# ---- 11: the wide AIR ---------------------------------------------------------------------------------------------------------------
def negated(interactions):
    """the same interactions with every multiplicity negated: the receiver of everything `interactions` sends"""
    inter, spans, bc = (np.asarray(x).copy() for x in interactions)
    inter, spans, out, new_spans = inter.reshape(-1, 3), spans.reshape(-1, 2), [], []
    firsts = set(inter[:, 2].tolist())
    for k, (off, ln) in enumerate(spans.tolist()):
        code = bc[off:off + ln].tolist() + ([5] if k in firsts else [])
        new_spans.append((len(out), len(code)))
        out += code
    return inter, np.array(new_spans, np.uint32), np.array(out, np.uint32)


@BOTH_PATHS
def test_the_wide_air(gpu, monkeypatch, interpret):
    torch, prover = gpu
    from tests import _oracle_cases as oc

    set_path(monkeypatch, interpret)
    flat, W, lh, _, _, it = oc.synthetic("C2", (1 << 14) - 5, seed=0)
    H = 1 << lh
    cols = flat.reshape(W, H)
    want = bm.verdicts([(cols, it)])
    snd = prover.Prover(W, *NO_CONS, num_queries=2, interactions=it)
    assert snd.logup_path() == (1 if interpret else 2)
    trace = to_dev(torch, flat)
    summaries, _ = prover.check_segment_buses([(snd, trace.data_ptr(), lh)], tuple_cap=0)
    assert [(s["bus"], s["n_active"], s["status"] == 0) for s in summaries] == [(b, n, ok) for b, (n, ok) in sorted(want.items())]
    assert sum(s["n_active"] for s in summaries) > 1 << 20
    # with a receiver of everything it sends (the same trace, multiplicities negated) every bus balances ...
    it_neg = negated(it)
    rcv = prover.Prover(W, *NO_CONS, num_queries=2, interactions=it_neg)
    copy = trace.clone()
    seg = [(snd, trace.data_ptr(), lh), (rcv, copy.data_ptr(), lh)]
    summaries, tuples = prover.check_segment_buses(seg)
    assert all(s["status"] == 0 for s in summaries) and tuples == []
    assert [(s["bus"], s["n_active"]) for s in summaries] == [(b, 2 * n) for b, (n, _) in sorted(want.items())]
    # ... until one cell of the receiver's copy changes: exactly the tuples of that row that read the cell are named
    plain, uses = plain_column_uses(it)
    inter = np.asarray(it[0]).reshape(-1, 3)
    col, row = None, 777
    for c, where in sorted(plain.items()):
        i = where[0][0]
        if uses[c] == 1 and len(where) == 1 and bm.tally([(cols[:, row:row + 1], bm_select(it, i))])[1][int(inter[i, 0]) % P] == 1:
            col, (i_t, arg_t) = c, where[0]
            break
    assert col is not None
    bump_cell(copy, col * H + row, 1 << 25)
    torch.cuda.synchronize()
    summaries, tuples = prover.check_segment_buses(seg)
    bus_t = int(inter[i_t, 0])
    assert [s["bus"] for s in summaries if s["status"] == 1] == [bus_t]
    key = next(k for k in bm.tally([(cols[:, row:row + 1], bm_select(it, i_t))])[0])
    moved = list(key[2])
    moved[arg_t] = (moved[arg_t] + (1 << 25)) % P
    mult = bm.tally([(cols[:, row:row + 1], bm_select(it, i_t))])[0][key][0]
    got = sorted((t["args"], t["net_multiplicity"]) for t in tuples)
    assert got == sorted([(list(key[2]), mult), (moved, (P - mult) % P)])
    sent = [t for t in tuples if t["args"] == list(key[2])][0]
    assert sent["air"] == 0 and (sent["interaction"], sent["row"]) <= (i_t, row)
    for p in (snd, rcv):
        p.close()


def bm_select(interactions, i):
    """the interaction table restricted to interaction i"""
    inter, spans, bc = interactions
    return np.asarray(inter).reshape(-1, 3)[i:i + 1], spans, bc
