"""Applying APC calls without a GPU: the numpy restatement of tests/_apc_sources_ref.py against the chips' own dummy
traces (oracle.original_chips.expand_dummy_traces) on the chained execution, bus conservation between the original AIRs and residuals
plus sources, the statuses the restatement raises, and every refusal of the two C entry points that needs neither a prover nor a GPU."""
import ctypes as C

import numpy as np
import pytest

from oracle import original_chips as ooc
from tests import _apc_sources_ref as ref
from tests import _bus_multiset as bm
from tests import _chained_vm as vm
from tests import _execution_states_ref as sref


def host_airs(ex, rec):
    """the instruction AIRs of the chained execution in kind order, as tests.test_empirical_gpu.host_airs builds them"""
    from powdr_amd import synth

    traces = ooc.expand_dummy_traces(ex.table, rec, ex.rbs)
    kinds = sorted(traces)
    return kinds, [(traces[k], synth.reference_air_programs(ooc.KIND_NAMES[k])[2]) for k in kinds]


def chained_calls(calls):
    """A (one block) on call 0, B (two blocks) on the call pairs 1 .. calls - 2, the last call uncovered"""
    n = len(vm.BLOCK)
    return [n, 2 * n], [(0, 0, n)] + [(1, k * n, (k + 2) * n) for k in range(1, calls - 1, 2)]


@pytest.fixture(scope="module")
def chained():
    ex = vm.Execution(64, seed=3)
    kinds, airs = host_airs(ex, ex.rec)
    cycles, calls = chained_calls(64)
    return ex, kinds, airs, cycles, calls, ref.apply(airs, cycles, calls, min_log_height=2)


def test_the_chained_execution_gives_the_chips_own_traces(chained):
    ex, kinds, airs, cycles, calls, got = chained
    assert calls == [(0, 0, 10)] + [(1, 10 * k, 10 * k + 20) for k in range(1, 63, 2)] and got["positions"] == 640
    want_a = ooc.expand_dummy_traces(ex.table, ex.rec[:, [0]], ex.rbs)
    want_b = ooc.expand_dummy_traces(ex.table, ex.rec[:, 1:63], ex.rbs)  # call j of B = the block's calls 2j + 1 and 2j + 2: rbs doubles
    want_r = ooc.expand_dummy_traces(ex.table, ex.rec[:, [63]], ex.rbs)
    assert sorted(got["sources"]) == [(a, air) for a in (0, 1) for air in range(len(kinds))] and sorted(got["residuals"]) == list(range(len(kinds)))
    for air, k in enumerate(kinds):
        m, rbs = got["sources"][(0, air)]
        assert rbs == ex.rbs[k] and m.shape == want_a[k].shape and (m == want_a[k]).all(), ooc.KIND_NAMES[k]
        m, rbs = got["sources"][(1, air)]
        assert rbs == 2 * ex.rbs[k] and m.shape == want_b[k].shape and (m == want_b[k]).all(), ooc.KIND_NAMES[k]
        m, rows = got["residuals"][air]
        assert rows == ex.rbs[k] and m.shape == want_r[k].shape and (m == want_r[k]).all(), ooc.KIND_NAMES[k]
    # the layout of A is the block's own: instruction i lies in the AIR of its kind at the block's air_row
    air_of_kind = {k: air for air, k in enumerate(kinds)}
    block = [(air_of_kind[int(ins["kind"])], int(ins["air_row"])) for ins in ex.table]
    assert got["layout"][0] == (1, block)
    assert got["layout"][1] == (31, block + [(air, row + ex.rbs[kinds[air]]) for air, row in block])


def test_buses_are_conserved_at_16_calls():
    ex = vm.Execution(16, seed=3)
    kinds, airs = host_airs(ex, ex.rec)
    cycles, calls = chained_calls(16)
    got = ref.apply(airs, cycles, calls)
    pieces = [(m, airs[air][1]) for air, (m, _) in sorted(got["residuals"].items())] + [(m, airs[air][1]) for (_, air), (m, _) in sorted(got["sources"].items())]
    before, active_before = bm.tally(airs)
    after, active_after = bm.tally(pieces)
    assert active_before == active_after and len(active_before) > 3
    assert {k: (e[0], e[2]) for k, e in before.items()} == {k: (e[0], e[2]) for k, e in after.items()}
    assert sum(rows for _, rows in got["residuals"].values()) == len(vm.BLOCK)


def test_statuses_11_and_12_by_the_restatement():
    ex = sref.Execution(40, seed=2)
    airs = ex.airs()
    pos, part = ref.where(airs)
    assert part == [0, 1] and len(pos) == 40 and {a for a, _ in pos} == {0, 1}
    with pytest.raises(ref.Status) as e:
        ref.apply(airs, [3, 2], [(0, 0, 3), (1, 5, 7), (0, 38, 41), (1, 41, 43)])
    assert (e.value.status, e.value.info) == (11, 2)
    assert ref.apply(airs, [3], [(0, 37, 40)])["layout"][0][0] == 1  # to == N is a call
    # two calls of one APC whose k-th rows lie in different AIRs: the smallest such position is named
    p = next(i for i in range(1, 40) if pos[i][0] != pos[0][0])
    q = next(i for i in range(p + 1, 40) if pos[i][0] != pos[0][0])
    with pytest.raises(ref.Status) as e:
        ref.apply(airs, [1], [(0, 0, 1), (0, q, q + 1)])
    assert (e.value.status, e.value.info) == (12, q)
    with pytest.raises(ref.Status) as e:
        ref.apply(airs, [1], [(0, 0, 1), (0, p, p + 1), (0, q, q + 1)])
    assert (e.value.status, e.value.info) == (12, p)
    from powdr_amd import apc_sources as aps

    assert "call 2" in str(aps.ApcSourcesError(11, 2)) and "position 17" in str(aps.ApcSourcesError(12, 17)) and aps.STATUS[11] and aps.STATUS[12]


def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import apc_sources as aps
    from powdr_amd import prover

    job = lambda **kw: aps.PwGatherJob(**{**dict(src=256, h_in=8, width=3, idx=512, out=1024, h_out=4), **kw})
    gather = lambda *jobs: aps.lib.pw_trace_gather_rows((aps.PwGatherJob * len(jobs))(*jobs), len(jobs))
    assert aps.lib.pw_trace_gather_rows(None, 0) == 0 and aps.lib.pw_trace_gather_rows(None, 1) == -1
    for null in ("src", "idx", "out"):
        assert gather(job(**{null: None})) == -1, null
    for bad in (0, 3, 6, 12, (1 << 20) + 1):
        assert gather(job(h_in=bad)) == -1 and gather(job(h_out=bad)) == -1, bad
    assert gather(job(h_in=1 << 32)) == -1 and gather(job(h_out=1 << 33)) == -1
    assert gather(job(width=0)) == -1 and gather(job(width=1 << 32)) == -1
    assert gather(job(), job(width=0)) == -1  # any job of the call
    with pytest.raises(ValueError, match="malformed"):
        aps.gather_rows([aps.GatherJob(256, 8, 0, 512, 1024, 4)])

    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    recs = (prover.PwSegmentAir * 2)()
    u32, u64 = lambda *v: (C.c_uint32 * len(v))(*v), lambda *v: (C.c_uint64 * len(v))(*v)

    def sources(recs=recs, seg=None, n_airs=0, bus=0, cycles=u32(3, 2), n_apcs=2, ids=u32(0, 1, 0), start=u64(0, 3, 5), end=u64(3, 5, 8), n_calls=3, mlh=0,
                out=C.byref(out), status=C.byref(status), info=C.byref(info)):
        return aps.lib.pw_apc_sources_from_traces(recs, seg, n_airs, bus, cycles, n_apcs, ids, start, end, n_calls, mlh, 0, out, status, info)

    for null in ("out", "status", "info", "cycles", "ids", "start", "end"):
        assert sources(**{null: None}) == -1, null
    assert sources(recs=None, n_airs=2) == -1 and sources(n_airs=2) == -1  # (a NULL prover: refused with the AIR list)
    assert sources(bus=sref.P) == -1
    assert sources(n_airs=2, seg=u32(0, 1)) == -1  # two segment numbers
    assert sources(ids=u32(0, 2, 0)) == -1  # apc_id >= n_apcs
    assert sources(cycles=u32(3, 0), ids=u32(0, 0, 0), start=u64(0, 3, 6), end=u64(3, 6, 9)) == -1  # cycle_count == 0, even of an APC without calls
    assert sources(end=u64(3, 6, 8)) == -1 and sources(end=u64(3, 4, 8)) == -1 and sources(start=u64(0, 3, 9), end=u64(3, 5, 8)) == -1  # a wrong call length
    assert sources(start=u64(5, 3, 0), end=u64(8, 5, 3)) == -1  # unsorted
    assert sources(start=u64(0, 2, 5), end=u64(3, 4, 8)) == -1  # overlapping
    assert sources(start=u64(0, 3, 3), end=u64(3, 5, 6)) == -1  # two calls at one position
    assert sources(mlh=32) == -1
    for f in (lambda: aps.apply_calls([], [(0, 0, 3), (0, 2, 5)], [3]), lambda: aps.apply_calls([], [aps.ApcCall(1, 0, 3)], [aps.Apc(0, 3, 1)])):
        with pytest.raises(ValueError, match="malformed"):
            f()
