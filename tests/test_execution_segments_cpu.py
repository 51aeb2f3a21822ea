"""Cutting an execution into segments without a GPU: the restatement of tests/_execution_segments_ref.py against a brute
force over every set of allowed cuts (valid, and no valid cut has fewer segments), the jumps of the padded height, every refusal of the
C entry point that needs neither a prover nor a GPU, and the argument checks of `cut`."""
import ctypes as C

import numpy as np
import pytest

from tests import _execution_segments_ref as ref
from tests import _execution_states_ref as sref


def random_case(rng, with_calls, with_cells):
    n = int(rng.integers(1, 13))
    air_of = rng.integers(0, 3, size=n).tolist()
    calls, at = [], 0
    while with_calls and at < n:
        at += int(rng.integers(0, 3))
        length = int(rng.integers(1, 5))
        if at + length > n:
            break
        calls.append((int(rng.integers(0, 2)), at, at + length))
        at += length
    width = {0: 3, 1: 7, 2: 1, ("apc", 0): 11, ("apc", 1): 2}
    limits = dict(max_log_height=int(rng.integers(0, 3)), min_log_height=0, max_cells=0)
    if with_cells:
        limits["min_log_height"] = int(rng.integers(0, limits["max_log_height"] + 1))
        limits["max_cells"] = int(rng.integers(1, 60))
    return ref.classes(air_of, calls), ref.allowed(n, calls), width, limits


@pytest.mark.parametrize("with_cells", [False, True])
@pytest.mark.parametrize("with_calls", [False, True])
def test_the_greedy_cut_is_valid_and_no_valid_cut_has_fewer_segments(with_calls, with_cells):
    rng = np.random.default_rng([0x5e9, with_calls, with_cells])
    cut, refused = 0, 0
    for _ in range(150):
        cls, ok, width, lim = random_case(rng, with_calls, with_cells)
        fewest = ref.fewest_segments(cls, ok, width, **lim)
        try:
            bounds, _ = ref.cut(cls, ok, width, **lim)
        except ref.Status as e:
            # status 13 at b: no allowed q > b fits from b. (Another cut set may still exist — the greedy prefix is not the only one —
            # but then the definition's own sequence b_s does not: it is the definition, not the brute force, that the device restates.)
            assert e.status == 13 and not any(ok[q] and ref.fits(cls, width, e.info, q, **lim) for q in range(e.info + 1, len(cls) + 1))
            refused += 1
            continue
        assert bounds[0] == 0 and bounds[-1] == len(cls) and all(p < q and ok[q] for p, q in zip(bounds, bounds[1:]))
        assert all(ref.fits(cls, width, p, q, **lim) for p, q in zip(bounds, bounds[1:]))
        # greedy: the next allowed position after a cut no longer fits
        for p, q in zip(bounds, bounds[1:]):
            assert not any(ok[r] and ref.fits(cls, width, p, r, **lim) for r in range(q + 1, len(cls) + 1))
        assert fewest == len(bounds) - 1
        cut += 1
    assert cut > 50 and (refused > 0) == with_cells


def test_a_cut_set_may_exist_where_nothing_fits_only_under_max_cells():
    """without max_cells a single class row always fits (cap >= 1) and a call's start is always allowed: status 13 cannot happen"""
    cls, ok = ref.classes([0, 0, 0, 0], [(0, 1, 4)]), ref.allowed(4, [(0, 1, 4)])
    assert ref.cut(cls, ok, {0: 1, ("apc", 0): 1}, 0)[0] == [0, 4]  # (one row of AIR 0, one of the APC)
    assert ref.cut(cls, ok, {0: 1, ("apc", 0): 9}, 0, max_cells=10)[0] == [0, 4] and ref.cut(cls, ok, {0: 1, ("apc", 0): 9}, 0, max_cells=9)[0] == [0, 1, 4]
    with pytest.raises(ref.Status) as e:
        ref.cut(cls, ok, {0: 1, ("apc", 0): 9}, 0, max_cells=8)
    assert (e.value.status, e.value.info) == (13, 1)
    with pytest.raises(ref.Status) as e:
        ref.cut([0] * 5, [True] * 6, {0: 1}, 0, max_segments=3)
    assert (e.value.status, e.value.info) == (14, 3)


def test_the_padded_height_jumps_at_a_power_of_two_and_one_more():
    assert [ref.padded(n) for n in (0, 1, 2, 3, 4, 5, 8, 9)] == [0, 1, 2, 4, 4, 8, 8, 16]
    assert [ref.padded(n, 2) for n in (0, 1, 4, 5)] == [0, 4, 4, 8]
    # width 5, min_log_height 1: n rows cost 5 * padded(n): 10, 10, 20, 20, 40 — a budget of 20 holds 4 rows, of 39 too, of 40 holds 8
    for budget, rows in ((9, None), (10, 2), (19, 2), (20, 4), (39, 4), (40, 8)):
        cls = [0] * 20
        if rows is None:
            with pytest.raises(ref.Status):
                ref.cut(cls, [True] * 21, {0: 5}, 4, min_log_height=1, max_cells=budget)
        else:
            assert ref.cut(cls, [True] * 21, {0: 5}, 4, min_log_height=1, max_cells=budget)[0][1] == rows, budget
    # the height cap alone: 2^k rows fit, one more does not
    for k in range(4):
        assert ref.cut([0] * 20, [True] * 21, {0: 5}, k)[0][1] == 1 << k


def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import execution_segments as es
    from powdr_amd import prover

    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    recs = (prover.PwSegmentAir * 2)()
    u32, u64 = lambda *v: (C.c_uint32 * len(v))(*v), lambda *v: (C.c_uint64 * len(v))(*v)
    lim = lambda mx=5, mn=0, cells=0, segs=0: C.byref(es.PwSegmentLimits(mx, mn, cells, segs))

    def segs(recs=recs, seg=None, n_airs=0, bus=0, cycles=u32(3, 2), widths=u32(4, 4), n_apcs=2, ids=u32(0, 1, 0), start=u64(0, 3, 5), end=u64(3, 5, 8), n_calls=3,
             limits=lim(), out=C.byref(out), status=C.byref(status), info=C.byref(info)):
        return es.lib.pw_execution_segments_from_traces(recs, seg, n_airs, bus, 0, cycles, widths, n_apcs, ids, start, end, n_calls, limits, 0, out, status, info)

    for null in ("out", "status", "info", "cycles", "ids", "start", "end", "limits"):
        assert segs(**{null: None}) == -1, null
    assert segs(recs=None, n_airs=2) == -1 and segs(n_airs=2) == -1  # (a NULL prover: refused with the AIR list)
    assert segs(bus=sref.P) == -1
    assert segs(n_airs=2, seg=u32(0, 1)) == -1  # two segment numbers
    assert segs(ids=u32(0, 2, 0)) == -1  # apc_id >= n_apcs
    assert segs(cycles=u32(3, 0), ids=u32(0, 0, 0), start=u64(0, 3, 6), end=u64(3, 6, 9)) == -1  # cycle_count == 0
    assert segs(end=u64(3, 6, 8)) == -1 and segs(end=u64(3, 4, 8)) == -1  # a wrong call length
    assert segs(start=u64(5, 3, 0), end=u64(8, 5, 3)) == -1  # unsorted
    assert segs(start=u64(0, 2, 5), end=u64(3, 4, 8)) == -1  # overlapping
    assert segs(limits=lim(mx=32)) == -1 and segs(limits=lim(mx=3, mn=4)) == -1
    assert segs(limits=lim(cells=100), widths=None) == -1 and segs(limits=lim(cells=100), widths=u32(4, 0)) == -1
    assert es.lib.pw_execution_segments_rows(None, 0, 0, None, None, None) == -1 and es.lib.pw_execution_segments_read_lists(None, None, None) == -1
    es.lib.pw_execution_segments_destroy(None)
    stats = es.last_stats()
    assert set(stats) == set(es.STATS) and stats["scratch_bytes"] == 0


def test_cut_checks_its_arguments():
    from powdr_amd import execution_segments as es

    with pytest.raises(ValueError, match="malformed"):
        es.cut([], 5, 0, calls=[(0, 0, 3), (0, 2, 5)], apcs=[3])  # overlapping calls
    with pytest.raises(ValueError, match="malformed"):
        es.cut([], 3, 0, min_log_height=4)
    with pytest.raises(ValueError, match="malformed"):
        es.cut([], 32, 0)
    with pytest.raises(ValueError, match="malformed"):
        es.cut([], 5, 0, calls=[es.ApcCall(0, 0, 3)], apcs=[es.Apc(0, 3, 1)], max_cells=10)  # no widths under max_cells
    with pytest.raises(ValueError, match="without apcs"):
        es.cut([], 5, 0, calls=[(0, 0, 3)])
    with pytest.raises(ValueError, match="one width per APC"):
        es.cut([], 5, 0, apcs=[3, 4], apc_widths=[7])
    with pytest.raises(ValueError, match="out of range"):
        es.cut([], -1, 0)
    with pytest.raises(ValueError, match="out of range"):
        es.cut([], 5, 1 << 32)
    e = es.ExecutionSegmentsError(13, 17)
    assert (e.status, e.info) == (13, 17) and "position 17" in str(e) and "call 2" in str(es.ExecutionSegmentsError(11, 2))
    assert all(es.STATUS[s] for s in (2, 4, 7, 11, 13, 14))
