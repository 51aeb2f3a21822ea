"""apply_calls on the GPU against the restatement of tests/_apc_sources_ref.py: every source and residual matrix word
for word, layouts, rows kept and heights; the statuses; and the chained execution from select_calls through apply_calls to the APC
trace generator and the bus check."""
import ctypes as C

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _apc_sources_ref as ref
from tests import _execution_states_ref as sref

pytestmark = pytest.mark.gpu
BODY = 12  # the program of the state logs: pcs 0, 4 .. 44 in a loop, with jumps back to 0


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def program_log(n, seed, air_of_pc=lambda pc: int((pc // 4) % 3 == 1), place_seed=1):
    """The rows of sref.Execution(n) with the pcs of a program — a loop of BODY instructions that now and then jumps back to its start — so
    that the AIR of a row is a function of its pc, as with real chips. -> (host AIRs: the rows at random places of two state-log AIRs of
    different heights, final pc)"""
    ex = sref.Execution(n, seed=seed)
    rng = np.random.default_rng([seed, n, 0xa9c])
    pcs, at = [], 0
    for _ in range(n + 1):
        pcs.append(4 * at)
        at = 0 if rng.integers(0, 8) == 0 else (at + 1) % BODY
    rows = [(pcs[i], ts, pcs[i + 1], nts, acc) for i, (_, ts, _, nts, acc) in enumerate(ex.rows)]
    it = sref.state_log_interactions(ex.n_access)
    place = np.random.default_rng([place_seed, n])
    host = []
    for air, extra in ((0, 1), (1, 0)):
        part = [r for r in rows if air_of_pc(r[0]) == air]
        log_h = max(1, (max(len(part), 2) - 1).bit_length()) + extra
        host.append((sref.state_log(part, ex.n_access, log_h=log_h, places=place.permutation(1 << log_h)[:len(part)]), it))
    return host, pcs[n]


def stretch(start, length, priority=1):
    """the APC of the program's instructions start .. start + length - 1: its path is pinned by pc constraints"""
    from powdr_amd import apc_calls as ac

    return ac.Apc(4 * start, length, priority, [ac.Constraint(ac.Pc(k), ac.Number(4 * ((start + k) % BODY))) for k in range(1, length)])


def seeded_apcs(seed):
    rng = np.random.default_rng([seed, 0x5eed])
    return [stretch(int(rng.integers(0, BODY)), int(rng.integers(1, 8)), int(rng.integers(0, 3))) for _ in range(3)]


def same(got, want, host):
    """the handle against the restatement: everything"""
    assert got.positions == want["positions"] and got.n_airs == len(host)
    assert [(l.n_calls, l.instructions) for l in got.layout] == want["layout"]
    source_bytes = 0
    for a in range(got.n_apcs):
        for air in range(got.n_airs):
            s, w = got.source(a, air), want["sources"].get((a, air))
            if w is None:
                assert s.height == 0 and s.ptr is None, (a, air)
                continue
            m, rbs = w
            assert (s.width, s.height, s.rbs) == (m.shape[0], m.shape[1], rbs) and s.ptr, (a, air)
            assert (om.from_monty(got.read_source(a, air)) == m).all(), (a, air)
            source_bytes += 4 * m.size
    residual_bytes = 0
    for air in range(got.n_airs):
        r, w = got.residual(air), want["residuals"].get(air)
        if w is None:
            assert r is None and got.read_residual(air) is None
            continue
        m, rows = w
        assert (r.rows, 1 << r.log_height) == (rows, m.shape[1]) and r.ptr, air
        assert (om.from_monty(got.read_residual(air)) == m).all(), air
        residual_bytes += 4 * m.size
    assert (got.source_bytes, got.residual_bytes) == (source_bytes, residual_bytes)


def run(gpu, host, final_pc, apcs, calls=None, min_log_height=0, **kw):
    """select_calls (unless the calls are given), apply_calls, the comparison -> (calls, the restatement's result)"""
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import Segment

    s = Segment(gpu, host)
    try:
        if calls is None:
            with ac.select_calls(s.seg, apcs, final_pc=final_pc) as chosen:
                calls = [tuple(c) for c in chosen.calls]
        want = ref.apply(host, [getattr(a, "cycle_count", a) for a in apcs], calls, min_log_height=min_log_height)
        with aps.apply_calls(s.seg, calls, apcs, min_log_height=min_log_height, **kw) as got:
            same(got, want, host)
            stats = aps.last_stats()
            assert stats["scratch_bytes"] == 0 and stats["covered"] == got.covered == sum(e - b for _, b, e in calls)
            assert stats["gather_jobs"] == len(want["sources"]) + len(want["residuals"]) and stats["peak_bytes"] >= got.source_bytes + got.residual_bytes
        assert aps.last_stats()["scratch_bytes"] == 0
    finally:
        s.close()
    return calls, want


@pytest.mark.parametrize("min_log_height", [0, 5])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 1025])
def test_state_logs_with_the_calls_select_calls_chose(gpu, n, min_log_height):
    host, final_pc = program_log(n, seed=n + 1)
    calls, want = run(gpu, host, final_pc, seeded_apcs(n), min_log_height=min_log_height)
    assert all(m.shape[1] >= 1 << min_log_height for m, _ in list(want["sources"].values()) + list(want["residuals"].values()))
    if n == 1025:
        assert len(calls) > 20 and len({a for a, _, _ in calls}) >= 2 and len({air for _, air in want["sources"]}) == 2
    if n == 0:
        assert calls == [] and all(rows == 0 for _, rows in want["residuals"].values())


def test_zero_calls_leave_the_active_rows_compacted(gpu):
    host, final_pc = program_log(300, seed=4)
    _, want = run(gpu, host, final_pc, seeded_apcs(4), calls=[])
    assert want["sources"] == {} and sum(rows for _, rows in want["residuals"].values()) == 300
    for air, (m, rows) in want["residuals"].items():
        cols = host[air][0]
        assert (m[:, :rows] == cols[:, cols[0] == 1]).all() and not m[:, rows:].any()  # (is_valid is column 0)


@pytest.mark.parametrize("min_log_height", [0, 5])
def test_every_position_covered_leaves_empty_residuals(gpu, min_log_height):
    from powdr_amd import apc_calls as ac

    host, final_pc = program_log(200, seed=6)
    apcs = [ac.Apc(4 * k, 1, 1) for k in range(BODY)]
    calls, want = run(gpu, host, final_pc, apcs, min_log_height=min_log_height)
    assert len(calls) == 200
    for m, rows in want["residuals"].values():
        assert rows == 0 and m.shape[1] == 1 << min_log_height and not m.any()


def test_an_apc_that_alternates_between_the_airs(gpu):
    host, final_pc = program_log(400, seed=7, air_of_pc=lambda pc: (pc // 4) % 2)
    calls, want = run(gpu, host, final_pc, [stretch(2, 6, 1), stretch(9, 5, 1)])
    assert want["layout"][0][1] == [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2), (1, 2)] and want["layout"][0][0] > 3
    assert want["layout"][1][1] == [(1, 0), (0, 0), (1, 1), (0, 1), (1, 2)] and want["layout"][1][0] > 3  # (instructions 9, 10, 11, 0, 1)
    assert want["sources"][(0, 0)][1] == 3 and want["sources"][(0, 1)][1] == 3 and want["sources"][(1, 0)][1] == 2 and want["sources"][(1, 1)][1] == 3


def test_the_row_order_does_not_change_a_source(gpu):
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import Segment

    apcs, seen = seeded_apcs(8), []
    for place_seed in (1, 2):
        host, final_pc = program_log(500, seed=8, place_seed=place_seed)
        s = Segment(gpu, host)
        try:
            with ac.select_calls(s.seg, apcs, final_pc=final_pc) as chosen, aps.apply_calls(s.seg, chosen, apcs) as got:
                seen.append(([tuple(l) for l in got.layout], {(a, air): got.read_source(a, air).tobytes() for a in range(3) for air in range(2)},
                             [got.residual(air).rows for air in range(2)]))
        finally:
            s.close()
    assert seen[0] == seen[1] and any(seen[0][1].values()) and sum(l[0] for l in seen[0][0]) > 10


def test_statuses_11_and_12(gpu):
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import Segment

    host = sref.Execution(40, seed=2).airs()  # rows in the two AIRs at random: calls of one APC disagree
    pos, _ = ref.where(host)
    p = next(i for i in range(1, 40) if pos[i][0] != pos[0][0])
    q = next(i for i in range(p + 1, 40) if pos[i][0] != pos[0][0])
    s = Segment(gpu, host)
    try:
        def status(cycles, calls, **kw):
            try:
                ref.apply(host, cycles, calls)
                want = None
            except ref.Status as e:
                want = (e.status, e.info)
            try:
                aps.apply_calls(s.seg, calls, cycles, **kw).close()
                got = None
            except aps.ApcSourcesError as e:
                got = (e.status, e.info)
            assert got == want and aps.last_stats()["scratch_bytes"] == 0
            return got

        assert status([3, 2], [(0, 0, 3), (1, 5, 7), (0, 38, 41), (1, 41, 43)]) == (11, 2)
        assert status([3], [(0, 37, 40)]) is None  # to == N is a call
        assert status([1], [(0, 0, 1), (0, q, q + 1)]) == (12, q)
        assert status([1], [(0, 0, 1), (0, p, p + 1), (0, q, q + 1)]) == (12, p)  # the smaller of two
        assert status([1], [(0, 0, 1), (0, q, q + 1), (0, 40, 41)]) == (11, 2)  # 11 before 12
    finally:
        s.close()


def test_statuses_7_and_4_come_first_and_an_air_without_the_bridge_takes_no_part(gpu):
    from powdr_amd import apc_sources as aps
    from tests import _empirical_ref as eref
    from tests.test_bus_check_gpu import Segment

    it = eref.block_log_interactions()
    rows = [(pc, 10 + t, [7 + t]) for t, pc in enumerate([0, 4, 8, 0, 4])]
    late = [(0, 0, 2), (0, 4, 6)]  # the second call ends after the 5 positions: status 11 wherever 7 and 4 do not come first

    def status(host, calls, **kw):
        s = Segment(gpu, host)
        try:
            aps.apply_calls(s.seg, calls, [2], **kw).close()
        except aps.ApcSourcesError as e:
            assert aps.last_stats()["scratch_bytes"] == 0  # (7 and 4 are raised after the index stage allocated)
            return e.status, e.info
        finally:
            s.close()

    assert status([(eref.block_log(rows, 1), it)], late) == (11, 1)
    assert status([(eref.block_log(rows + [(4, 12, [0])], 1), it)], late) == (4, 12)  # a duplicate time key
    twice = eref.block_log(rows + [(4, 12, [0])], 1)
    twice[0, 3] = 2
    assert status([(eref.block_log(rows, 1), it), (twice, it)], late) == (7, (1 << 32) | 3)  # a multiplicity of 2: before the duplicate
    assert status([(eref.block_log(rows, 1), it)], late, bus=1) == (11, 0)  # no AIR on the bus: no position at all
    # an AIR whose interactions lie on another bus: no residual, no source, and its rows are no positions
    other = (eref.block_log([(0, 11, [1]), (4, 13, [2])], 1), eref.block_log_interactions(bus=3))
    host = [other, (eref.block_log(rows, 1, log_h=4, places=[9, 2, 15, 0, 7]), it)]
    _, want = run(gpu, host, 0, [2], calls=[(0, 1, 3)])
    assert sorted(want["residuals"]) == [1] and want["residuals"][1][1] == 3 and sorted(want["sources"]) == [(0, 1)] and want["positions"] == 5
    assert (want["sources"][(0, 1)][0][3] == [8, 9]).all() and (want["residuals"][1][0][3][:3] == [10, 11, 7]).all()  # the data column: rows 0, 7, 9
    s = Segment(gpu, host)
    try:
        with aps.apply_calls(s.seg, [], [2], bus=1) as got:  # nobody on the bus: an empty result
            assert got.positions == 0 and [got.residual(a) for a in range(2)] == [None, None] and got.layout == [(0, [])]
    finally:
        s.close()


def test_status_2_and_a_run_inside_the_bytes_it_names(gpu):
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import Segment

    host, final_pc = program_log(1025, seed=9)
    apcs = [stretch(0, 3), stretch(5, 4)]
    calls, _ = run(gpu, host, final_pc, apcs)
    assert len(calls) > 20
    s = Segment(gpu, host)
    try:
        with pytest.raises(aps.ApcSourcesError) as e:
            aps.apply_calls(s.seg, calls, apcs, scratch_bytes=1 << 16)
        assert e.value.status == 2 and e.value.info > 1 << 16 and aps.last_stats()["scratch_bytes"] == 0
        with aps.apply_calls(s.seg, calls, apcs, scratch_bytes=e.value.info) as got:
            assert got.covered == sum(b - a for _, a, b in calls)
        stats = aps.last_stats()
        assert 0 < stats["peak_bytes"] <= e.value.info and stats["scratch_bytes"] == 0
    finally:
        s.close()
    run(gpu, host, final_pc, apcs, calls=calls, scratch_bytes=e.value.info)


# ---- the chained execution: select_calls -> apply_calls -> the APC trace generator, the bus check ------------------------------------------
def tracegen(torch, h_airs, n_airs, subs, height, width, calls):
    """powdr_apc_tracegen_host_tables without a device table -> the output, canonical [width, height]"""
    from powdr_amd import abi

    f = abi.lib.powdr_apc_tracegen_host_tables
    f.restype = C.c_int
    f.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
    out = torch.full((width * height,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    subs = np.ascontiguousarray(subs, dtype=np.int32)
    torch.cuda.synchronize()
    assert f(out.data_ptr(), height, None, h_airs, n_airs, subs.ctypes.data, len(subs), calls) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).reshape(width, height)


def test_the_chained_execution_from_calls_to_apc_traces(gpu):
    from oracle import original_chips as ooc
    from powdr_amd import abi
    from powdr_amd import apc_calls as ac
    from powdr_amd import apc_sources as aps
    from powdr_amd import original_chips as pc
    from tests import _chained_vm as vm
    from tests.test_apc_calls_gpu import to_apcs
    from tests.test_apc_sources_cpu import chained_calls, host_airs
    from tests.test_empirical_gpu import device_airs

    torch, prover = gpu
    ex = vm.Execution(64, seed=3)
    n, bit = len(vm.BLOCK), ex.initial[(1, 8)][0] & 1
    apcs = to_apcs([(vm.START_PC, n, 1, [(("reg", 0, 2, 0), ("num", bit))]), (vm.START_PC, 2 * n, 2, [(("reg", n, 2, 0), ("num", bit))])])
    kinds, host = host_airs(ex, ex.rec)
    cycles, want_calls = chained_calls(64)
    seg, keep, names = device_airs(gpu, ex.table, ex.rec, 64)
    selected = {0: device_airs(gpu, ex.table, ex.rec[:, [0]], 1), 1: device_airs(gpu, ex.table, ex.rec[:, 1:63], 62)}
    try:
        assert [names[a] for a in range(len(seg))] == [ooc.KIND_NAMES[k] for k in kinds]
        with ac.select_calls(seg, apcs, final_pc=ex.end[0], limb_bits=1, registers=dict(n_regs=8)) as chosen, \
                aps.apply_calls(seg, chosen, apcs, min_log_height=2) as got:
            assert [tuple(c) for c in chosen.calls] == want_calls
            # sources and residuals: the chips' own traces of the selected records, as in the CPU test
            want = ref.apply(host, cycles, want_calls, min_log_height=2)
            same(got, want, host)
            expand = lambda rec: ooc.expand_dummy_traces(ex.table, rec, ex.rbs)
            for air, k in enumerate(kinds):
                assert (om.from_monty(got.read_source(0, air)) == expand(ex.rec[:, [0]])[k]).all()
                assert (om.from_monty(got.read_source(1, air)) == expand(ex.rec[:, 1:63])[k]).all()
                assert (om.from_monty(got.read_residual(air)) == expand(ex.rec[:, [63]])[k]).all()
            # the APC trace generator on every cell of the APC's instructions: through the handle's tables, and on the traces
            # powdr_original_airs_expand makes of the selected records (B's call = two calls of the block: rbs doubles, the second block's
            # rows come rbs later)
            itab = pc.InstructionTable(vm.BLOCK, [True] * n, vm.START_PC)
            for a, n_calls, height in ((0, 1, 4), (1, 31, 32)):
                block = [(int(ins["kind"]), int(ins["air_row"])) for ins in ex.table]
                instrs = block if a == 0 else block + [(k, row + ex.rbs[k]) for k, row in block]
                cells = [(i, col) for i, (k, _) in enumerate(instrs) for col in range(pc.WIDTHS[k])]
                mine = tracegen(torch, got.original_airs(a), len(got.source_airs(a)), got.substs(a, [(i, col, c) for c, (i, col) in enumerate(cells)]), height,
                                len(cells), n_calls)
                sel_seg = selected[a][0]
                h_airs = (abi.OriginalAir * len(kinds))(*[abi.OriginalAir(pc.WIDTHS[k], 1 << sel_seg[air][2], sel_seg[air][1], (a + 1) * ex.rbs[k])
                                                          for air, k in enumerate(kinds)])
                subs = [(kinds.index(instrs[i][0]), col, instrs[i][1], c) for c, (i, col) in enumerate(cells)]
                theirs = tracegen(torch, h_airs, len(kinds), subs, height, len(cells), n_calls)
                assert (mine == theirs).all() and mine[:, :n_calls].any() and len(itab) == n
            # the buses: residuals plus sources carry what the original segment carried
            pieces = got.residual_segment(seg)
            for a in (0, 1):
                for air in got.source_airs(a):
                    s = got.source(a, air)
                    pieces.append((seg[air][0], s.ptr, s.height.bit_length() - 1))
            strip = lambda t: {k: v for k, v in t.items() if k not in ("air", "interaction", "row")}
            before_s, before_t = prover.check_segment_buses(seg, tuple_cap=1 << 16)
            after_s, after_t = prover.check_segment_buses(pieces, tuple_cap=1 << 16)
            assert before_s == after_s and len(before_s) > 3 and [strip(t) for t in before_t] == [strip(t) for t in after_t]
        assert aps.last_stats()["scratch_bytes"] == 0
    finally:
        for group in [seg] + [v[0] for v in selected.values()]:
            for p, _, _ in group:
                p.close()
