"""Cutting an execution into segments on the GPU against the restatement of tests/_execution_segments_ref.py: every field
exact — the cuts, the first time key and pc of every segment, the calls' ranges, every class count, every row list word for word with
its padding and alignment — the statuses, determinism, and the chained execution cut without and with calls: every segment closed,
checked, proven and chained, and every segment's calls applied.

The synthetic traces are state logs as in tests/test_apc_direct_gpu.py: a strictly periodic program (position i runs instruction
i mod period, whose AIR is pattern[i mod period]) at random rows of two AIRs of different widths (41 and 17 columns) and heights,
padding rows interleaved, rows permuted against time. No row accesses memory: the cut reads the execution bridge alone."""
import functools
import types

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _apc_sources_ref as aref
from tests import _execution_segments_ref as ref
from tests import _execution_states_ref as sref

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5
FILL_I32 = int(np.uint32(FILL).view(np.int32))
W0, W1 = 41, 17  # the widths of the two state logs (3 and 1 access slots)


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


@functools.lru_cache(maxsize=None)
def log(n, pattern=(0, 1, 0, 0), place_seed=1, seed=5):
    """-> (host AIRs [(cols canonical, interactions)], final pc): n positions, shared and left unchanged"""
    period = len(pattern)
    rng = np.random.default_rng([seed, n, 0x5e95])
    ts = (1000 + np.cumsum(rng.integers(1, 4, size=n + 1))).tolist()
    rows = [(4 * (i % period), ts[i], 4 * ((i + 1) % period), ts[i + 1], []) for i in range(n)]
    place = np.random.default_rng([place_seed, n, 0xd1])
    host = []
    for air, (n_access, extra) in enumerate(((3, 1), (1, 0))):
        part = [r for i, r in enumerate(rows) if pattern[i % period] == air]
        log_h = max(2, (max(len(part), 2) - 1).bit_length()) + extra
        host.append((sref.state_log(part, n_access, log_h=log_h, places=place.permutation(1 << log_h)[:len(part)]), sref.state_log_interactions(n_access)))
    assert [len(c) for c, _ in host] == [W0, W1]
    return tuple(host), 4 * (n % period)


class Dev:
    """host AIRs on the device (tests.test_bus_check_gpu.Segment) with their Montgomery words on the host"""

    def __init__(self, gpu, host):
        from tests.test_bus_check_gpu import Segment

        self.host = list(host)
        self.s = Segment(gpu, self.host)
        self.seg = self.s.seg
        self.monty = [om.to_monty(np.ascontiguousarray(cols)).reshape(cols.shape) for cols, _ in host]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.s.close()


def same(got, want, n_apcs=0, n_airs=2):
    """the handle against the restatement: everything"""
    from powdr_amd import execution_segments as es

    S = len(want["bounds"]) - 1
    assert (got.n_segments, got.positions, got.n_airs, got.n_apcs) == (S, want["positions"], n_airs, n_apcs)
    assert got.bounds == want["bounds"] and got.starts == want["starts"] and got.final_pc == want["final_pc"] and got.first_call == want["first_call"]
    assert got.heights == want["heights"]
    lists = got.read_lists()
    assert sorted(lists) == sorted(want["lists"])  # an AIR without rows in a segment has no list
    words = 0
    for key, w in want["lists"].items():
        ptr, rows, lh = got.rows(*key)
        assert ptr % 16 == 0 and rows == sum(x != ref.PAD for x in w) and 1 << lh == len(w), key
        assert lists[key].tolist() == w, key
        words += (len(w) + 3) & ~3
    assert got.list_bytes == 4 * words
    for s in range(S):
        for air in range(n_airs):
            assert (got.rows(s, air) is None) == ((s, air) not in want["lists"])
    stats = es.last_stats()
    assert (stats["segments"], stats["classes"], stats["snapped_cuts"], stats["scratch_bytes"]) == (S, n_airs + n_apcs, want["snapped"], 0)
    assert stats["peak_bytes"] >= got.list_bytes
    return stats


def run(gpu, host, final_pc, max_log_height, calls=(), cycles=(), apc_widths=None, **kw):
    """cut on the device and by the restatement, compared -> (the restatement's result, the stats)"""
    from powdr_amd import execution_segments as es

    want = ref.segments(host, final_pc, max_log_height, calls, apc_widths or [0] * len(cycles), **{k: v for k, v in kw.items() if k != "scratch_bytes"})
    with Dev(gpu, host) as d, es.cut(d.seg, max_log_height, final_pc, calls=list(calls), apcs=list(cycles), apc_widths=apc_widths, **kw) as got:
        assert got.covered == sum(e - b for _, b, e in calls)
        stats = same(got, want, len(cycles))
    assert es.last_stats()["scratch_bytes"] == 0
    return want, stats


def status_of(gpu, host, final_pc, max_log_height, calls=(), cycles=(), apc_widths=None, **kw):
    """the status of the device and of the restatement, equal -> (status, info) or None; no scratch is held afterwards"""
    from powdr_amd import execution_segments as es

    ref_kw = {k: v for k, v in kw.items() if k not in ("scratch_bytes", "bus")}
    try:
        ref.segments(host, final_pc, max_log_height, calls, apc_widths or [0] * len(cycles), bus=kw.get("bus", 0), **ref_kw)
        want = None
    except ref.Status as e:
        want = (e.status, e.info)
    with Dev(gpu, host) as d:
        try:
            es.cut(d.seg, max_log_height, final_pc, calls=list(calls), apcs=list(cycles), apc_widths=apc_widths, **kw).close()
            got = None
        except es.ExecutionSegmentsError as e:
            got = (e.status, e.info)
    assert es.last_stats()["scratch_bytes"] == 0
    if "scratch_bytes" not in kw:
        assert got == want
    return got


# ---- without calls --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_log_height", [0, 1, 5])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, (1 << 16) + 1])
def test_state_logs_of_every_size(gpu, n, max_log_height):
    host, final_pc = log(n)
    want, stats = run(gpu, host, final_pc, max_log_height)
    S = len(want["bounds"]) - 1
    assert stats["cell_probes"] == 0 and want["snapped"] == 0
    if n == 0:
        assert S == 0 and want["bounds"] == [0] and want["lists"] == {}
    if max_log_height == 0:  # every class row its own segment: AIR 0 has three of four positions, so a segment is 0 | 0 1 | 0 (1 or 2 positions)
        assert all(h in ({0: 1}, {1: 1}, {0: 1, 1: 1}) for h in want["heights"]) and n // 2 <= S <= n
    if max_log_height == 5 and n > 1000:
        assert S == -(-(n - (n + 2) // 4) // 32)  # AIR 0 (every position but i = 1 mod 4) fills first: 32 of its rows per segment


def test_a_class_exactly_at_the_cap_at_the_end_and_one_more(gpu):
    for n, segments in ((63, 1), (64, 1), (65, 2)):  # pattern 0 1: AIR 0 has 32, 32, 33 rows
        host, final_pc = log(n, pattern=(0, 1))
        want, _ = run(gpu, host, final_pc, 5)
        assert len(want["bounds"]) - 1 == segments and sum(h.get(0, 0) for h in want["heights"]) == (n + 1) // 2
    assert want["bounds"] == [0, 64, 65] and want["heights"][1] == {0: 1}


# ---- calls ------------------------------------------------------------------------------------------------------------------------------
def test_calls_at_the_ends_back_to_back_and_an_apc_that_fills_first(gpu):
    host, final_pc = log(300)
    cases = {
        "none": ([], []),
        "at_position_0": ([(0, 0, 7)], [7]),
        "ending_at_n": ([(0, 293, 300)], [7]),
        "back_to_back": ([(0, 10 + 7 * j, 17 + 7 * j) for j in range(20)] + [(1, 150, 153), (1, 153, 156), (0, 156, 163)], [7, 3]),
        "one_position_calls": ([(0, j, j + 1) for j in range(0, 300, 2)], [1]),
    }
    for name, (calls, cycles) in cases.items():
        for mlh in (1, 3):
            want, _ = run(gpu, host, final_pc, mlh, calls, cycles)
            ok = ref.allowed(300, calls)
            assert all(ok[b] for b in want["bounds"]), name  # no call is cut
            assert sum(h.get(("apc", a), 0) for h in want["heights"] for a in range(len(cycles))) == len(calls), name
    # an APC class reaching the cap before any AIR: everything covered by calls of 4 positions, a cap of 2 calls
    calls = [(0, 4 * j, 4 * j + 4) for j in range(75)]
    want, _ = run(gpu, host, final_pc, 1, calls, [4])
    assert want["bounds"] == list(range(0, 300, 8)) + [300] and all(set(h) == {("apc", 0)} for h in want["heights"])
    assert want["first_call"] == list(range(0, 75, 2)) + [75]
    assert all(len([x for x in want["lists"][(s, 0)] if x != ref.PAD]) == (6 if s < 37 else 3) for s in range(38))  # covered rows are in the lists


def test_no_bound_falls_inside_a_call(gpu):
    """fits(b, q) changes only where position q - 1 has a class — an uncovered position or a call's first — so the largest q that fits
    is such a position: always an allowed cut, under the height cap and under the cell budget alike. The library still checks every
    cut against the call table and counts the cuts it had to move to a call's start; the restatement counts the same by walking. Both
    say 0, and no call is cut."""
    host, final_pc = log(300, pattern=(0, 1))
    # the height bound next to a call: AIR 0 (the even positions) has 4 rows in [0, 8), a call covers [8, 40), its fifth row is position 40
    calls = [(0, 8, 40)]
    want, stats = run(gpu, host, final_pc, 2, calls, [32])
    assert want["bounds"][:3] == [0, 40, 48] and want["snapped"] == 0 and want["heights"][0] == {0: 4, 1: 4, ("apc", 0): 1}
    # the cell budget ends at a call's first position: its APC row is the one that does not fit
    want, stats = run(gpu, host, final_pc, 5, calls, [32], [1000], max_cells=W0 * 4 + W1 * 4 + 999)
    assert want["bounds"][:2] == [0, 8] and want["snapped"] == 0 and stats["cell_probes"] > 0
    # random calls of two APCs under random budgets
    rng = np.random.default_rng(77)
    segments = 0
    for _ in range(6):
        calls, at = [], 0
        while True:
            a = int(rng.integers(0, 2))
            at += int(rng.integers(0, 9))
            if at + (5, 9)[a] > 300:
                break
            calls.append((a, at, at + (5, 9)[a]))
            at += (5, 9)[a]
        want, stats = run(gpu, host, final_pc, 3, calls, [5, 9], [60, 7], max_cells=int(rng.integers(300, 900)))
        ok = ref.allowed(300, calls)
        assert want["snapped"] == 0 and stats["cell_probes"] > 0 and all(ok[b] for b in want["bounds"])
        segments += len(want["bounds"]) - 1
    assert segments > 30


@pytest.mark.parametrize("n_apcs", [65, 257])
def test_many_apc_classes(gpu, n_apcs):
    host, final_pc = log(1025)
    calls = [(j % n_apcs, 3 * j, 3 * j + 2) for j in range(340)]  # APC j mod n_apcs, two positions each, one uncovered between them
    want, stats = run(gpu, host, final_pc, 1, calls, [2] * n_apcs, list(range(1, n_apcs + 1)), max_cells=5000)
    assert stats["classes"] == 2 + n_apcs and stats["cell_probes"] > 0 and len(want["bounds"]) > 10
    assert len({c for h in want["heights"] for c in h}) == 2 + n_apcs
    want, _ = run(gpu, host, final_pc, 0, calls, [2] * n_apcs)  # the cap alone: one row per class
    assert all(set(h.values()) == {1} for h in want["heights"])


# ---- max_cells --------------------------------------------------------------------------------------------------------------------------
def test_the_cell_budget(gpu):
    host, final_pc = log(300, pattern=(0, 1))
    # binding before the heights
    free, _ = run(gpu, host, final_pc, 5)
    want, stats = run(gpu, host, final_pc, 5, max_cells=W0 * 8 + W1 * 4)
    assert len(want["bounds"]) > len(free["bounds"]) and stats["cell_probes"] > len(want["bounds"]) - 1 and max(max(h.values()) for h in want["heights"]) < 32
    # binding exactly at a jump of the padded height: 8 + 8 rows cost 464 cells, and so do 5 + 5; 5 + 4 cost 396
    assert W0 * 8 + W1 * 8 == 464
    assert run(gpu, host, final_pc, 5, max_cells=464)[0]["bounds"][:2] == [0, 16]
    assert run(gpu, host, final_pc, 5, max_cells=463)[0]["bounds"][:2] == [0, 9]
    # min_log_height makes a one-row class expensive: a row of AIR 0 costs 41 * 32, with a row of AIR 1 beside it 58 * 32
    want, _ = run(gpu, host, final_pc, 5, min_log_height=5, max_cells=W0 * 32)
    assert want["bounds"] == list(range(301)) and all(len(w) == 32 for w in want["lists"].values())
    want, _ = run(gpu, host, final_pc, 5, min_log_height=5, max_cells=(W0 + W1) * 32)
    assert want["bounds"][:3] == [0, 64, 128]
    # a sum past 2^32: an APC of 2^32 - 1 columns; four calls are padded to 4 rows, the fifth to 8
    wide = (1 << 32) - 1
    calls = [(0, 10 * j, 10 * j + 2) for j in range(30)]
    want, _ = run(gpu, host, final_pc, 5, calls, [2], [wide], max_cells=4 * wide + (W0 + W1) * 32)
    assert want["heights"][0][("apc", 0)] == 4 and want["bounds"][1] == 40
    want, _ = run(gpu, host, final_pc, 5, calls, [2], [wide], max_cells=(1 << 64) - 1)
    assert want["heights"][0][0] == 32


# ---- the row lists and the gathered segments --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_log_height, min_log_height", [(0, 0), (1, 0), (1, 1), (4, 0), (5, 3)])
def test_gathered_segments_equal_numpy_indexing_of_the_originals(gpu, max_log_height, min_log_height):
    from powdr_amd import execution_segments as es

    torch = gpu[0]
    host, final_pc = log(257)
    calls = [(0, 40, 47), (0, 47, 54)] if max_log_height == 4 else []
    want = ref.segments(host, final_pc, max_log_height, calls, [3], min_log_height=min_log_height)
    with Dev(gpu, host) as d, es.cut(d.seg, max_log_height, final_pc, calls=calls, apcs=[7] if calls else None, min_log_height=min_log_height) as got:
        same(got, want, 1 if calls else 0)
        heights = set()
        for s in range(got.n_segments):
            buffers = {air: torch.full((w << ((len(want["lists"][(s, air)]) - 1).bit_length()),), FILL_I32, dtype=torch.int32, device="cuda")
                       for air, w in ((0, W0), (1, W1)) if (s, air) in want["lists"]}
            torch.cuda.synchronize()
            out = got.segment(s, buffers=buffers)
            assert [air for air, _, _, _ in out] == sorted(buffers)
            for air, pr, t, lh in out:
                idx = np.array(want["lists"][(s, air)], np.int64)
                expect = np.where(idx[None, :] == ref.PAD, 0, d.monty[air][:, np.minimum(idx, d.monty[air].shape[1] - 1)]).astype(np.uint32)
                assert t.data_ptr() == buffers[air].data_ptr() and pr is d.seg[air][0] and 1 << lh == len(idx)
                assert (t.cpu().numpy().view(np.uint32) == expect).all(), (s, air)
                heights.add(len(idx))
            fresh = got.segment(s)  # and into tensors of its own
            assert all(torch.equal(a[2], b[2]) for a, b in zip(out, fresh))
        if max_log_height <= 1 and min_log_height == 0:
            assert heights == {1} if max_log_height == 0 else heights == {1, 2}  # the gather's word path
        with pytest.raises(ValueError, match="buffer of AIR 0"):
            got.segment(0, buffers={0: torch.zeros(3, dtype=torch.int32, device="cuda")})
        with pytest.raises(IndexError):
            got.rows(got.n_segments, 0)
        with pytest.raises(IndexError):
            got.rows(0, 2)


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_status_2_and_a_run_inside_the_bytes_it_names(gpu):
    from powdr_amd import execution_segments as es

    host, final_pc = log(1025)
    calls = [(0, 9 * j, 9 * j + 5) for j in range(100)]
    got = status_of(gpu, host, final_pc, 3, calls, [5], [9], max_cells=4000, scratch_bytes=1 << 16)
    assert got is not None and got[0] == 2 and got[1] > 1 << 16
    want, stats = run(gpu, host, final_pc, 3, calls, [5], [9], max_cells=4000, scratch_bytes=got[1])
    assert 0 < stats["peak_bytes"] <= got[1] and len(want["bounds"]) > 10
    assert run(gpu, host, final_pc, 3, calls, [5], [9], max_cells=4000)[0] == want  # the default bound: the same cut


def test_statuses_7_4_11_13_14_in_that_order(gpu):
    from tests import _empirical_ref as eref

    it = eref.block_log_interactions()
    rows = [(pc, 10 + t, [7 + t]) for t, pc in enumerate([0, 4, 8, 0, 4])]
    late = [(0, 0, 2), (0, 4, 6)]  # the second call ends after the 5 positions
    good = [(eref.block_log(rows, 1), it)]
    assert status_of(gpu, good, 8, 5, late, [2]) == (11, 1)
    assert status_of(gpu, [(eref.block_log(rows + [(4, 12, [0])], 1), it)], 8, 5, late, [2]) == (4, 12)  # a duplicate time key: before 11
    twice = eref.block_log(rows + [(4, 12, [0])], 1)
    twice[0, 3] = 2
    assert status_of(gpu, good + [(twice, it)], 8, 5, late, [2]) == (7, (1 << 32) | 3)  # a multiplicity of 2: before the duplicate
    assert status_of(gpu, good, 8, 5, late, [2], bus=1) == (11, 0)  # no AIR on the bus: no position, so no call fits
    assert status_of(gpu, good, 8, 5, [], [], bus=1) is None  # and without calls an empty cut
    # 11 before 13 and 14
    assert status_of(gpu, good, 8, 0, late, [2], [9], max_cells=1, max_segments=1) == (11, 1)
    width = len(good[0][0])
    # 13: not even the first row fits; then a call whose APC row does not fit, named at its start
    assert status_of(gpu, good, 8, 5, max_cells=width - 1) == (13, 0)
    assert status_of(gpu, good, 8, 5, [(0, 2, 4)], [2], [100], max_cells=99) == (13, 2)
    assert status_of(gpu, good, 8, 5, [(0, 2, 4)], [2], [100], max_cells=100) is None
    # 14: the position reached when the segments run out; 13 and 14 in the order the cuts meet them
    assert status_of(gpu, good, 8, 0, max_segments=2) == (14, 2)
    assert status_of(gpu, good, 8, 0, max_segments=4) == (14, 4) and status_of(gpu, good, 8, 0, max_segments=5) is None
    assert status_of(gpu, good, 8, 0, [(0, 2, 4)], [2], [100], max_cells=99, max_segments=2) == (14, 2)
    assert status_of(gpu, good, 8, 0, [(0, 2, 4)], [2], [100], max_cells=99, max_segments=3) == (13, 2)
    host, final_pc = log(1025)
    assert status_of(gpu, host, final_pc, 0, max_segments=700)[0] == 14  # (status_of compares the position reached with the restatement's)


# ---- determinism and order independence -----------------------------------------------------------------------------------------------
def test_two_runs_are_identical_and_the_row_order_does_not_matter(gpu):
    from powdr_amd import execution_segments as es

    calls = [(j % 3, 11 * j, 11 * j + 4) for j in range(90)]
    seen = []
    for place_seed in (1, 1, 2):
        host, final_pc = log(1025, place_seed=place_seed)
        with Dev(gpu, host) as d, es.cut(d.seg, 3, final_pc, calls=calls, apcs=[4, 4, 4], apc_widths=[5, 50, 500], max_cells=3000) as got:
            lists = {k: v.tobytes() for k, v in got.read_lists().items()}
            seen.append((got.bounds, got.starts, got.heights, got.first_call, got.final_pc, lists))
    assert seen[0] == seen[1] and len(seen[0][0]) > 20
    assert seen[0][:5] == seen[2][:5] and seen[0][5] != seen[2][5] and sorted(seen[0][5]) == sorted(seen[2][5])  # other rows, the same cut


# ---- the chained execution ------------------------------------------------------------------------------------------------------------------
def three_alu_block():
    """tests/_chained_vm.BLOCK without its XOR (three BaseAlu instructions per call), the jump back adjusted"""
    from oracle import original_chips as oc
    from tests import _chained_vm as vm

    block = [list(ins) for ins in vm.BLOCK if ins[0] != 514]
    assert len(block) == 9 and block[-1][0] == 560
    block[-1][3] = oc.P - 32
    return block


@pytest.fixture(scope="module")
def chained():
    from tests import _chained_vm as vm

    ex = vm.Execution(48, seed=5, block=three_alu_block())
    airs = ex.instruction_airs()
    assert sum(int(ins["kind"]) == int(ex.table[0]["kind"]) for ins in ex.table) == 3  # BaseAlu: 3 rows per call
    return ex, airs


def piece_of(ex, airs, part):
    """what tests.test_system_airs_gpu.Closed takes, for a gathered segment: part = ExecutionSegments.segment(s)"""
    from tests.test_bus_check_gpu import from_dev

    made = [(airs[air][0], from_dev(t).reshape(pr.width, 1 << lh), airs[air][2]) for air, pr, t, lh in part]
    return types.SimpleNamespace(instruction_airs=lambda: made, program_table=ex.program_table, start_pc=ex.start_pc)


def test_the_chained_execution_cut_closed_proven_and_chained(gpu, chained, monkeypatch):
    torch, prover = gpu
    from powdr_amd import execution_segments as es
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa
    from tests import _memory_tree_ref as tref
    from tests import test_system_airs_gpu as tsa
    from tests.test_memory_merkle_gpu import H, closed_with, constants, statement
    from tests.test_memory_tree_gpu import leaf_of

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex, airs = chained
    host = [(t, programs[2]) for _, t, programs in airs]
    leaves = dict(leaf_of(loc, word) for loc, (word, _) in ex.initial.items())
    keys0 = np.array(sorted(leaves), np.uint64)
    pay0 = np.array([leaves[int(x)] for x in keys0], np.uint32)
    with Dev(gpu, host) as d, es.cut(d.seg, 5, ex.end[0]) as got:
        want = ref.segments(host, ex.end[0], 5)
        S = got.n_segments
        assert got.bounds == want["bounds"] and got.heights == want["heights"] and got.starts == want["starts"]
        assert S >= 3 and got.positions == 48 * 9 and any(b % 9 for b in got.bounds[1:-1])  # a segment that starts mid-call
        assert got.starts[0] == ex.start and got.final_pc == ex.end[0]
        tree = mt.MemoryTree(H)
        assert tree.load(keys0, pay0) == (0, 0)
        closed, segments = [], []
        for s in range(S):
            c = closed_with(gpu, piece_of(ex, airs, got.segment(s)), public_connector=True, poseidon2=True, memory_tree=tree)
            closed.append(c)
            summaries, tuples = prover.check_segment_buses(c.seg)
            assert [(x["bus"], x["status"]) for x in summaries] == [(b, 0) for b in (0, 1, 2, 3, 5, 6, 7, 8, 9)] and tuples == []
            for a in c.airs:
                assert a["prover"].check_constraints(a["trace"].data_ptr(), a["log_h"]) == (0, None, None), (s, a["name"])
            pc0, ts0, pc1, ts1 = (int(x) for x in c.by_name("connector")["public"])
            assert (pc0, ts0) == got.starts[s]
            assert pc1 == (got.starts[s + 1][0] if s + 1 < S else got.final_pc) and (s + 1 == S or ts1 == got.starts[s + 1][1])
            g = statement(prover, c, prover.prove_segment(c.seg, logup=True))
            rc, total = prover.verify_segment(g["descs"], g["proof"], tsa.NQ, 0, True, check_balance=True, preprocessed=g["preprocessed"], public=g["public"])
            assert rc == 0 and not np.asarray(total).any()
            segments.append(g)
        names = [[a["name"] for a in c.airs] for c in closed]
        ci, mi = names[0].index("connector"), names[0].index("memory_merkle")
        assert all(n.index("connector") == ci and n.index("memory_merkle") == mi for n in names)
        assert prover.verify_segment_chain(segments, sa.connector_links(ci) + mt.memory_links(mi), tsa.NQ, 0) == (0, 0)
        last_root = tree.root().copy()
        for c in closed:
            c.close()
        tree.close()
    # the un-cut execution as one closed segment leaves the same memory
    whole = mt.MemoryTree(H)
    assert whole.load(keys0, pay0) == (0, 0)
    closed_with(gpu, ex, public_connector=True, poseidon2=True, memory_tree=whole).close()
    assert (whole.root() == last_root).all() and (last_root != tref.SparseTree(H, constants()).root()).any()
    whole.close()


def test_the_chained_execution_cut_with_calls_and_every_segment_applied(gpu, chained):
    torch, prover = gpu
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from powdr_amd import execution_segments as es
    from tests.test_bus_check_gpu import compare

    ex, airs = chained
    host = [(t, programs[2]) for _, t, programs in airs]
    apcs = [ac.Apc(ex.start_pc, 9, 1)]  # the whole block
    with Dev(gpu, host) as d:
        with ac.select_calls(d.seg, apcs, final_pc=ex.end[0]) as chosen:
            every = [tuple(c) for c in chosen.calls]
        assert every == [(0, 9 * j, 9 * j + 9) for j in range(48)]
        calls = [c for j, c in enumerate(every) if j % 5 != 2]  # ten calls stay with the original chips
        want = ref.segments(host, ex.end[0], 3, calls, [200])
        with es.cut(d.seg, 3, ex.end[0], calls=calls, apcs=apcs, apc_widths=[200]) as got:
            same(got, want, 1, len(host))
            S = got.n_segments
            assert S >= 4 and all(b % 9 == 0 for b in got.bounds) and max(h.get(("apc", 0), 0) for h in got.heights) == 8  # the APC class reaches the cap; no call is cut
            assert sum(len(got.calls(s)) for s in range(S)) == len(calls)
            for s in range(S):
                part = got.segment(s)
                seg_s = [(pr, t.data_ptr(), lh) for _, pr, t, lh in part]
                calls_s = got.calls(s)
                assert [tuple(c) for c in calls_s] == [(a, b - got.bounds[s], e - got.bounds[s]) for a, b, e in calls if got.bounds[s] <= b < got.bounds[s + 1]]
                # the two-step restatement: the segment by numpy indexing, then the calls applied to it
                host_s = []
                for air, _, _, _ in part:
                    idx = np.array(want["lists"][(s, air)], np.int64)
                    cols = host[air][0]
                    host_s.append((np.where(idx[None, :] == ref.PAD, 0, cols[:, np.minimum(idx, cols.shape[1] - 1)]).astype(np.uint32), host[air][1]))
                applied = aref.apply(host_s, [9], [tuple(c) for c in calls_s])
                with aps.apply_calls(seg_s, calls_s, apcs) as res:
                    assert res.layout[0].n_calls == got.heights[s].get(("apc", 0), 0) == applied["layout"][0][0]
                    for k, (air, _, _, _) in enumerate(part):
                        assert res.residual(k).rows == got.heights[s].get(air, 0) == applied["residuals"][k][1], (s, air)
                    pieces = res.residual_segment(seg_s)
                    compare(prover, pieces, [(applied["residuals"][k][0], host_s[k][1]) for k in range(len(part))])
    assert es.last_stats()["scratch_bytes"] == 0 and aps.last_stats()["scratch_bytes"] == 0
