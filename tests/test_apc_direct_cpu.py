"""Direct mode of applying APC calls without a GPU: the numpy restatement of tests/_apc_direct_ref.py — index lists,
then the definition as indexing — against the `_apc_tracegen` definition applied to the source matrices of tests/_apc_sources_ref.py on
the chained execution, and every refusal of pw_apc_sources_tracegen and pw_apc_sources_from_traces_flags that needs neither a prover nor
a GPU (a handle over no AIRs is made without one)."""
import ctypes as C

import numpy as np
import pytest

from tests import _apc_direct_ref as dref
from tests.test_apc_sources_cpu import chained  # noqa: F401  (the module's fixture: §5j's chained execution with §5s's call list)


def test_direct_traces_equal_tracegen_on_the_sources(chained):
    ex, kinds, airs, cycles, calls, applied = chained
    layout, index_lists = dref.lists(airs, cycles, calls)
    assert layout == applied["layout"] and sorted(index_lists) == sorted(applied["sources"])
    for key, (L, rbs) in index_lists.items():
        assert rbs == applied["sources"][key][1] and len(L) == layout[key[0]][0] * rbs and len(set(L.tolist())) == len(L)
    widths = [len(cols) for cols, _ in airs]
    rng = np.random.default_rng(0xd1)
    for apc, out_height in ((0, 4), (1, 32), (1, 128)):
        cells = dref.all_cells(layout, apc, widths)
        assert len(cells) == sum(widths[air] for air, _ in layout[apc][1])
        full = dref.traces(airs, layout, index_lists, apc, cells, out_height, len(cells))
        want = dref.from_sources(applied["sources"], layout, apc, cells, out_height, len(cells))
        n_calls = layout[apc][0]
        assert (full == want).all() and full[:, :n_calls].any() and not full[:, n_calls:].any()
        # a random quarter of the cells, scattered over the columns of a wider trace: the others keep the fill
        width = 2 * len(cells)
        pick = rng.permutation(len(cells))[:len(cells) // 4]
        cols = rng.permutation(width)[:len(pick)]
        some = [(cells[i][0], cells[i][1], int(c)) for i, c in zip(pick.tolist(), cols.tolist())]
        got = dref.traces(airs, layout, index_lists, apc, some, out_height, width)
        want = dref.from_sources(applied["sources"], layout, apc, some, out_height, width)
        untouched = np.setdiff1d(np.arange(width), cols)
        assert (got == want).all() and (got[untouched] == dref.FILL).all() and len(untouched) == width - len(some)
        assert (got[cols] == full[pick]).all()  # (all_cells numbers the APC columns as it lists the cells)


def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import apc_sources as aps
    from powdr_amd import prover
    from tests import _execution_states_ref as sref

    # ---- the flags entry: what pw_apc_sources_from_traces refuses, and any bit but PW_APC_SOURCES_DIRECT ----
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    recs = (prover.PwSegmentAir * 2)()
    u32, u64 = lambda *v: (C.c_uint32 * len(v))(*v), lambda *v: (C.c_uint64 * len(v))(*v)

    def sources(recs=recs, seg=None, n_airs=0, bus=0, cycles=u32(3, 2), n_apcs=2, ids=u32(0, 1, 0), start=u64(0, 3, 5), end=u64(3, 5, 8), n_calls=3, mlh=0, flags=1,
                out=C.byref(out), status=C.byref(status), info=C.byref(info)):
        return aps.lib.pw_apc_sources_from_traces_flags(recs, seg, n_airs, bus, cycles, n_apcs, ids, start, end, n_calls, mlh, 0, flags, out, status, info)

    for flags in (0, 1):
        for null in ("out", "status", "info", "cycles", "ids", "start", "end"):
            assert sources(flags=flags, **{null: None}) == -1, null
        assert sources(flags=flags, recs=None, n_airs=2) == -1 and sources(flags=flags, n_airs=2) == -1
        assert sources(flags=flags, bus=sref.P) == -1
        assert sources(flags=flags, n_airs=2, seg=u32(0, 1)) == -1
        assert sources(flags=flags, ids=u32(0, 2, 0)) == -1
        assert sources(flags=flags, end=u64(3, 6, 8)) == -1 and sources(flags=flags, start=u64(5, 3, 0), end=u64(8, 5, 3)) == -1
        assert sources(flags=flags, start=u64(0, 2, 5), end=u64(3, 4, 8)) == -1
        assert sources(flags=flags, mlh=32) == -1
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFF):
        assert sources(flags=flags, n_calls=0) == -1, flags
    with pytest.raises(ValueError, match="malformed"):
        aps.apply_calls([], [(0, 0, 3), (0, 2, 5)], [3], direct=True)

    # ---- pw_apc_sources_tracegen: a handle over no AIRs needs no GPU; its APCs have no calls ----
    tracegen, stats = aps.lib.pw_apc_sources_tracegen, aps.tracegen_last_stats
    good = (1, [(0, 0, 0), (1, 7, 2)], 4096, 4, 3)

    def refused(h, *jobs):
        recs, keep = aps.trace_jobs(list(jobs))
        return tracegen(h._h, recs, len(jobs)) == -1

    with aps.apply_calls([], [], [3, 2]) as plain, aps.apply_calls([], [], [3, 2], direct=True) as direct:
        assert not plain.direct and direct.direct and plain.index_bytes == direct.index_bytes == 0 and direct.source_bytes == 0
        assert aps.lib.pw_apc_sources_index_bytes(None) == 0
        recs, keep = aps.trace_jobs([good])
        assert tracegen(None, recs, 1) == -1 and tracegen(direct._h, None, 1) == -1
        assert tracegen(plain._h, recs, 1) == -1 and tracegen(plain._h, recs, 0) == -1  # a handle that is not direct
        with pytest.raises(ValueError, match="not direct"):
            plain.apc_traces([good])
        assert tracegen(direct._h, None, 0) == 0 and tracegen(direct._h, recs, 0) == 0 and stats()["jobs"] == 0  # no job: nothing to do
        apc, cells, ptr, height, width = good
        assert refused(direct, (2, cells, ptr, height, width))  # apc >= n_apcs
        assert refused(direct, (apc, [(2, 0, 0)], ptr, height, width)) and refused(direct, (0, [(3, 0, 0)], ptr, height, width))  # instr >= cycle_count
        assert refused(direct, (apc, [(0, 0, 3)], ptr, height, width))  # apc_col >= out_width
        assert refused(direct, (apc, [(0, 0, 1), (1, 5, 1)], ptr, height, width))  # two cells with one apc_col
        assert refused(direct, (apc, [(0, 0, 1), (0, 0, 1)], ptr, height, width))
        for bad in (0, 3, 6, 12, (1 << 20) + 1, 1 << 33):
            assert refused(direct, (apc, cells, ptr, bad, width)), bad  # out_height
        assert refused(direct, (apc, cells, ptr, height, 0))  # out_width == 0
        assert refused(direct, (apc, cells, None, height, width))  # d_out NULL
        null_cells = aps.PwApcTraceJob(apc, None, 2, ptr, height, width)
        assert tracegen(direct._h, C.pointer(null_cells), 1) == -1
        # the output matrices of two jobs overlap: 3 columns of 4 words are 48 bytes
        assert refused(direct, good, (0, [(0, 0, 0)], ptr + 44, height, width)) and refused(direct, (0, [(0, 0, 0)], ptr + 16, 4, 1), good)
        assert refused(direct, good, good)
        assert refused(direct, good, (apc, cells, ptr + 48, height, 0))  # any job of the call
        with pytest.raises(ValueError, match="malformed"):
            direct.apc_traces([(apc, cells, ptr, 12, width)])
        for f in (direct.original_airs, lambda a: direct.substs(a, [])):
            with pytest.raises(ValueError, match="apc_traces"):
                f(0)
        assert plain.substs(0, []).shape == (0, 4)
        assert stats()["scratch_bytes"] == 0
