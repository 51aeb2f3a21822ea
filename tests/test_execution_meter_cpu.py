"""The metered cut without a GPU: the restatement of tests/_execution_meter_ref.py against a brute force over every set
of allowed cuts (valid, greedy, no valid cut has fewer segments, status 13 exactly where nothing fits), the Merkle count against its
closed form, the jumps of padded_sys, every refusal of the metered entry point that needs neither a prover nor a GPU, and the argument
checks of `cut(system=)`."""
import ctypes as C

import numpy as np
import pytest

from tests import _execution_meter_ref as mref
from tests import _execution_segments_ref as ref
from tests import _execution_states_ref as sref

WIDTH = {0: 3, 1: 7, 2: 1, ("apc", 0): 11, ("apc", 1): 2}
CAPS = ("none", "boundary", "merkle", "poseidon2")


def random_case(rng, height, with_calls, with_cells, binding):
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
    keys_at = [rng.integers(0, 1 << height, size=int(rng.integers(0, 3))).tolist() for _ in range(n)]
    caps = [31, 31, 31]
    if binding != "none":
        # a boundary cap of 1 to 4 blocks; a Merkle cap around one path's H + 1 nodes, so that a single position may already pass it
        caps[CAPS.index(binding) - 1] = int(rng.integers(0, 3)) if binding == "boundary" else int(rng.integers(height // 2, height + 2)) + (binding == "poseidon2")
    lim = dict(max_log_height=int(rng.integers(0, 3)), height=height, caps=tuple(caps), sys_widths=(2, 1, 3), min_log_height=0, max_cells=0)
    if with_cells:
        lim["min_log_height"] = int(rng.integers(0, lim["max_log_height"] + 1))
        lim["max_cells"] = int(rng.integers(1, 60 + 100 * height))  # (one path of H + 1 nodes costs 3 * padded_sys(2 H + 2) cells and more)
    return ref.classes(air_of, calls), ref.allowed(n, calls), keys_at, lim


@pytest.mark.parametrize("binding", CAPS)
@pytest.mark.parametrize("with_cells", [False, True])
@pytest.mark.parametrize("with_calls", [False, True])
@pytest.mark.parametrize("height", [1, 4])
def test_the_greedy_cut_is_valid_and_no_valid_cut_has_fewer_segments(height, with_calls, with_cells, binding):
    rng = np.random.default_rng([0x5e95, height, with_calls, with_cells, CAPS.index(binding)])
    cut, refused, moved = 0, 0, 0
    for _ in range(60):
        cls, ok, keys_at, lim = random_case(rng, height, with_calls, with_cells, binding)
        fits = lambda p, q: mref.fits_sys(cls, keys_at, WIDTH, p, q, **lim)
        fewest = mref.fewest_segments(cls, ok, keys_at, WIDTH, **lim)
        try:
            bounds, heights, snapped = mref.cut(cls, ok, keys_at, WIDTH, **lim)
        except ref.Status as e:
            # status 13 at b: no allowed q > b fits from b — exactly there
            assert e.status == 13 and not any(ok[q] and fits(e.info, q) for q in range(e.info + 1, len(cls) + 1))
            refused += 1
            continue
        assert bounds[0] == 0 and bounds[-1] == len(cls) and all(p < q and ok[q] for p, q in zip(bounds, bounds[1:]))
        assert all(fits(p, q) for p, q in zip(bounds, bounds[1:]))
        for p, q in zip(bounds, bounds[1:]):  # greedy: no later allowed position fits
            assert not any(ok[r] and fits(p, r) for r in range(q + 1, len(cls) + 1))
        assert heights == [mref.counts(keys_at, p, q, height) for p, q in zip(bounds, bounds[1:])]
        assert fewest == len(bounds) - 1
        cut += 1
        moved += snapped
    assert cut >= 10
    if binding == "none" and not with_cells:
        assert refused == 0 and moved == 0  # §5v's remark holds while no system limit binds
    if binding in ("merkle", "poseidon2") and height == 4:
        assert refused > 0  # status 13 without max_cells: one position whose own paths pass the cap
    if binding != "none" and with_calls and not with_cells and height == 4:
        assert moved > 0  # a new block inside a call: the cut moves to the call's start


def test_the_merkle_count_is_the_closed_form():
    rng = np.random.default_rng(0xc105ed)
    for height in (1, 4, 30):
        for _ in range(40):
            keys = rng.integers(0, 1 << height, size=int(rng.integers(0, 9))).tolist()
            b, m, p = mref.counts([keys], 0, 1, height)
            assert b == len(set(keys)) and m == mref.merkle_closed_form(keys, height) and p == 2 * m
    assert mref.counts([[5]], 0, 1, 30) == (1, 31, 62) and mref.counts([[]], 0, 1, 30) == (0, 0, 0)
    assert mref.counts([[0, 1 << 29]], 0, 1, 30) == (2, 31 + 30, 122)  # keys that differ only in bit H - 1 share the root alone


def test_padded_sys_jumps():
    from powdr_amd import execution_segments as es

    want = {0: 0, 1: 2, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8, 9: 16}
    assert {n: mref.padded_sys(n) for n in want} == want and {n: es.padded_sys(n) for n in want} == want
    assert [mref.padded_sys(n, 2) for n in (0, 1, 4, 5)] == [0, 4, 4, 8] == [es.padded_sys(n, 2) for n in (0, 1, 4, 5)]
    # one AIR of width 1 and one access to a fresh block per position, tree of height 1, widths (10, 0, 0): n positions cost
    # padded(n) + 10 * padded_sys(n): 21 for one, 22 for two, 44 for three
    cls, ok, keys_at = [0] * 2, [True] * 3, [[0], [1]]
    run = lambda cells: mref.cut(cls, ok, keys_at, {0: 1}, 4, 1, (31, 31, 31), (10, 0, 0), max_cells=cells)[0]
    assert run(22) == [0, 2] and run(21) == [0, 1, 2]
    with pytest.raises(ref.Status) as e:
        run(20)
    assert (e.value.status, e.value.info) == (13, 0)


def test_the_widths_are_the_system_airs():
    from powdr_amd import execution_segments as es
    from powdr_amd import memory_tree, system_airs

    assert (es.BOUNDARY_WIDTH, es.MERKLE_WIDTH, es.POSEIDON2_WIDTH) == (system_airs.BOUNDARY_WIDTH, memory_tree.MERKLE_WIDTH, system_airs.POSEIDON2_WIDTH) == mref.WIDTHS
    assert es.SystemMeter().widths == mref.WIDTHS and es.SystemMeter().memory_bus == system_airs.BUS_MEMORY and es.SystemMeter().tree_height == 30


def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import execution_segments as es
    from powdr_amd import prover

    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    recs = (prover.PwSegmentAir * 2)()
    limits = C.byref(es.PwSegmentLimits(5, 0, 0, 0))

    def metered(meter, limits=limits, n_airs=0, out=C.byref(out)):
        return es.lib.pw_execution_segments_from_traces_metered(recs, None, n_airs, 0, 0, None, None, 0, None, None, None, 0, limits, meter, 0, out, C.byref(status),
                                                                C.byref(info))

    rec = lambda **kw: C.byref(es.SystemMeter(**kw).record(5))
    assert metered(None) == -1  # a NULL meter
    assert metered(rec(tree_height=0)) == -1 and metered(rec(tree_height=31)) == -1
    for k in range(3):
        caps = [31, 31, 31]
        caps[k] = 32
        assert metered(rec(max_log_height=tuple(caps))) == -1, k
    assert metered(rec(memory_bus=sref.P)) == -1
    assert metered(rec(), limits=None) == -1 and metered(rec(), out=None) == -1 and metered(rec(), n_airs=2) == -1  # what the unmetered call refuses
    es.lib.pw_execution_segments_read_system_heights(None, None)
    assert es.last_meter_stats() == dict.fromkeys(es.METER_STATS, 0) or set(es.last_meter_stats()) == set(es.METER_STATS)
    assert es.last_stats()["scratch_bytes"] == 0 and len(es.STATS) == 6


def test_cut_checks_its_arguments():
    from powdr_amd import execution_segments as es
    from powdr_amd import stage

    for bad in (dict(tree_height=0), dict(tree_height=31), dict(max_log_height=32), dict(max_log_height=(5, 32, 5)), dict(memory_bus=sref.P)):
        with pytest.raises(stage.Malformed, match="pw_execution_segments_from_traces_metered: malformed arguments"):
            es.cut([], 5, 0, system=es.SystemMeter(**bad))
    with pytest.raises(ValueError, match="three caps and three widths"):
        es.cut([], 5, 0, system=es.SystemMeter(max_log_height=(1, 2)))
    with pytest.raises(ValueError, match="three caps and three widths"):
        es.cut([], 5, 0, system=es.SystemMeter(widths=(1, 2, 3, 4)))
    with pytest.raises(ValueError, match="out of range"):
        es.cut([], 5, 0, system=es.SystemMeter(widths=(-1, 2, 3)))
    m = es.SystemMeter().record(7)
    assert list(m.max_log_height) == [7, 7, 7] and list(m.width) == [18, 55, 307] and (m.memory_bus, m.tree_height) == (1, 30)
    assert list(es.SystemMeter(max_log_height=3).record(7).max_log_height) == [3, 3, 3]
    assert list(es.SystemMeter(max_log_height=(1, 2, 3)).record(7).max_log_height) == [1, 2, 3]
    e = es.ExecutionSegmentsError(15, stage.pack_witness(3, 5, 9))
    assert str(e) == "pw_execution_segments: status 15, a memory-bus tuple that has no key (air 3, interaction 5, row 9)"
