"""Superblock detection without a GPU: the second route of tests/_execution_blocks_ref.py against the reference's own
unit cases (tests/golden/execution_blocks_unit_cases.json), the filters of `.blocks()`, the map order, every refusal that needs no GPU."""
import ctypes as C
import json
from pathlib import Path

import pytest

from tests import _execution_blocks_ref as ref

GOLDEN = json.loads((Path(__file__).parent / "golden" / "execution_blocks_unit_cases.json").read_text())


def test_find_non_overlapping_golden():
    for case in GOLDEN["find_non_overlapping"]:
        assert ref.find_non_overlapping(case["haystack"], case["needle"]) == case["indices"], case
    assert ref.find_non_overlapping(list("abababa"), list("aba")) == [0, 4]


def test_superblocks_in_run_golden():
    g = GOLDEN["superblocks_in_run"]
    counts = ref.superblocks_of([g["run"]], g["max_len"])
    assert len(counts) == g["n_superblocks"]
    assert [sum(1 for w in counts if len(w) == L + 1) for L in range(g["max_len"])] == g["n_by_length"]
    for c in g["counts"]:
        assert counts[tuple(c["start_pcs"])] == c["count"], c


def test_detect_superblocks_golden():
    g = GOLDEN["detect_superblocks"]
    got = ref.detect(g["execution"], g["blocks"], max_bb=g["max_bb"], pc_step=g["pc_step"])
    assert got["execution_bb_runs"] == [(tuple(r["start_pcs"]), r["count"]) for r in g["execution_bb_runs"]]
    for c in g["counts"]:
        assert got["superblock_counts"][tuple(c["start_pcs"])] == c["count"], c
    for absent in g["absent"]:
        assert tuple(absent) not in got["superblock_counts"]
    assert got["pc_count"] == {pc: g["execution"].count(pc) for pc in sorted(set(g["execution"]))}


def test_count_and_update_run_golden():
    for case in GOLDEN["count_and_update_run"]:
        assert ref.count_and_update_run(case["needle"], case["run"]) == (case["count"], case["sub_runs"]), case
    # over an execution: instances of one run count each, and what is left is per instance
    total, after = ref.count_and_update_execution([1, 2], [[1, 2, 3, 1, 2, 4], [3, 4, 5], [1, 2, 3, 1, 2, 4]])
    assert total == 4 and after == [[3], [4], [3, 4, 5], [3], [4]]


def test_the_walk_and_its_status_3():
    blocks = [(0, 3), (0x20, 1), (0x40, 2)]
    pcs = [0, 4, 8, 0x20, 0x40, 0x44, 0, 4, 8, 0x40]  # the last block is cut off by the end of the list: it counts
    got = ref.detect(pcs, blocks, max_bb=2)
    assert got["runs"] == [[0], [0x40, 0, 0x40]]
    assert got["superblock_counts"] == {(0,): 2, (0, 0x40): 1, (0x40,): 2, (0x40, 0): 1}
    for bad, where in (([4, 8], 0), ([0, 4, 8, 0x30], 3), ([0, 4, 12], 2), ([0, 4, 12, 0x30], 2), ([0, 8], 1), ([0x44], 0)):
        with pytest.raises(ref.Status) as e:
            ref.detect(bad, blocks)
        assert (e.value.status, e.value.info) == (3, where), bad
    with pytest.raises(ref.Status) as e:
        ref.detect([0, 4, 12], blocks, keys=[70, 80, 90])
    assert e.value.info == 90


def test_map_order_puts_a_prefix_before_its_extensions():
    from powdr_amd import execution_blocks as eb

    seqs = [(400,), (100, 200, 300), (100, 200), (100,), (100, 300), (100, 200, 100)]
    assert eb.lexicographic(seqs) == [(100,), (100, 200), (100, 200, 100), (100, 200, 300), (100, 300), (400,)]
    assert eb.lexicographic([[100, 200, 300], [400], [100, 200]]) == [(100, 200), (100, 200, 300), (400,)]
    got = ref.detect([100, 101, 200, 201, 300, 301, 400, 401, 100, 101, 200, 201], [(100, 2), (200, 2), (300, 2), (400, 2)], max_bb=3, pc_step=1)
    keys = list(got["superblock_counts"])
    assert keys == eb.lexicographic(keys) and keys.index((100, 200)) + 1 == keys.index((100, 200, 300)) < keys.index((400,))


def test_the_filters_of_blocks():
    from powdr_amd import execution_blocks as eb

    n = {100: 2, 200: 2, 400: 3}
    counts = {(400, 100): 1, (100,): 2, (200,): 2, (400,): 1, (100, 200): 2}
    assert eb.filter_blocks(counts, n) == [((100,), 2), ((100, 200), 2), ((200,), 2), ((400,), 1), ((400, 100), 1)]
    assert eb.filter_blocks(counts, n, exec_count_cutoff=2) == [((100,), 2), ((100, 200), 2), ((200,), 2)]
    assert eb.filter_blocks(counts, n, max_instructions=3) == [((100,), 2), ((200,), 2), ((400,), 1)]  # 4 and 5 instructions are too many
    assert eb.filter_blocks(counts, n, exec_count_cutoff=2, max_instructions=2) == [((100,), 2), ((200,), 2)]
    assert eb.filter_blocks(counts, n, exec_count_cutoff=0, max_instructions=0) == []


def test_refusals_before_any_gpu_call():
    from powdr_amd import empirical, prover
    from powdr_amd import execution_blocks as eb

    lib = eb.lib
    blocks = lambda *b: (empirical.PwBasicBlock * max(len(b), 1))(*[empirical.PwBasicBlock(s, n) for s, n in b])
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    somewhere = C.c_void_p(0x1000)  # never read: every call below returns before it touches the pcs

    def pcs(ptr, n, pc_step, blk, n_blk, max_bb=1, o=C.byref(out), s=C.byref(status), i=C.byref(info)):
        return lib.pw_execution_blocks_from_pcs(ptr, n, pc_step, blk, n_blk, max_bb, 0, o, s, i)

    def empty_result():
        assert status.value == 0 and out.value
        sizes = (C.c_uint64 * 6)()
        lib.pw_execution_blocks_sizes(out, sizes)
        assert list(sizes) == [0] * 6
        count = C.c_uint64(7)
        assert lib.pw_execution_blocks_count(out, (C.c_uint32 * 1)(0), 1, 1, C.byref(count)) == 0 and count.value == 0
        assert lib.pw_execution_blocks_count(out, None, 1, 0, C.byref(count)) == -1
        assert lib.pw_execution_blocks_count(out, (C.c_uint32 * 1)(0), 0, 0, C.byref(count)) == -1
        assert lib.pw_execution_blocks_count(out, (C.c_uint32 * 1)(0), 1, 0, None) == -1
        lib.pw_execution_blocks_destroy(out)

    # an empty execution: an empty result, no GPU needed
    assert pcs(None, 0, 4, blocks((0, 2)), 1) == 0
    empty_result()
    assert pcs(None, 0, 4, None, 0, max_bb=255) == 0
    empty_result()
    # NULL pointers
    assert pcs(None, 1, 4, blocks((0, 2)), 1) == -1
    assert pcs(somewhere, 1, 4, None, 1) == -1
    assert pcs(None, 0, 4, blocks(), 0, o=None) == -1
    assert pcs(None, 0, 4, blocks(), 0, s=None) == -1
    assert pcs(None, 0, 4, blocks(), 0, i=None) == -1
    # pc_step 0, max_bb 0 and above 255, 2^32 pcs
    assert pcs(None, 0, 0, blocks((0, 2)), 1) == -1
    assert pcs(None, 0, 4, blocks((0, 2)), 1, max_bb=0) == -1
    assert pcs(None, 0, 4, blocks((0, 2)), 1, max_bb=256) == -1
    assert pcs(somewhere, 2**32, 4, blocks((0, 2)), 1) == -1
    assert pcs(somewhere, 2**40, 4, blocks((0, 2)), 1) == -1
    # block tables: a zero count, unsorted, equal starts, overlapping, past 2^32
    for bad in ([(0, 0)], [(8, 1), (0, 1)], [(8, 1), (8, 1)], [(0, 3), (8, 1)], [(0xFFFFFFFC, 2)]):
        assert pcs(None, 0, 4, blocks(*bad), len(bad)) == -1, bad
    for good in ([(0, 2), (8, 1)], [(0xFFFFFFF8, 2)], [(0, 1), (4, 1), (8, 5)]):
        assert pcs(None, 0, 4, blocks(*good), len(good)) == 0, good
        lib.pw_execution_blocks_destroy(out)

    # the trace route: what pw_empirical_detect refuses, and max_bb
    none = (prover.PwSegmentAir * 1)()

    def traces(airs, n_airs, pc_step, blk, n_blk, max_bb=1, o=C.byref(out), s=C.byref(status), i=C.byref(info)):
        return lib.pw_execution_blocks_from_traces(airs, None, n_airs, 0, pc_step, blk, n_blk, max_bb, 0, o, s, i)

    assert traces(none, 0, 4, blocks((0, 2)), 1) == 0  # no AIRs: an empty result
    empty_result()
    assert traces(None, 1, 4, blocks(), 0) == -1
    assert traces(none, 0, 4, None, 1) == -1
    assert traces(none, 0, 4, blocks(), 0, o=None) == -1
    assert traces(none, 0, 4, blocks(), 0, s=None) == -1
    assert traces(none, 0, 4, blocks(), 0, i=None) == -1
    assert traces(none, 1, 4, blocks(), 0) == -1  # an entry without a prover
    assert traces(none, 0, 0, blocks((0, 2)), 1) == -1
    assert traces(none, 0, 4, blocks((0, 2)), 1, max_bb=0) == -1
    assert traces(none, 0, 4, blocks((0, 2)), 1, max_bb=256) == -1
    assert traces(none, 0, 4, blocks((0, 0)), 1) == -1
    # the wrapper
    with pytest.raises(Exception):
        eb.detect([], [(0, 2)], pc_step=0)
    with eb.detect([], [(0, 2)], max_bb=3) as e:
        assert e.pc_count == {} and e.execution_bb_runs == [] and e.superblock_counts == {} and e.blocks() == [] and e.count([0]) == 0
    with pytest.raises(ValueError):
        e.count([0])  # closed


def test_the_error_decodes_its_info():
    from powdr_amd import execution_blocks as eb

    assert "position 17" in str(eb.ExecutionBlocksError(3, 17))
    assert "segment 2, timestamp 9" in str(eb.ExecutionBlocksError(3, (2 << 32) | 9, from_traces=True))
    assert "4096 bytes needed" in str(eb.ExecutionBlocksError(2, 4096))
    assert "air 1, row 3" in str(eb.ExecutionBlocksError(7, (1 << 32) | 3, from_traces=True))
    e = eb.ExecutionBlocksError(6, 0)
    assert (e.status, e.info) == (6, 0)


def test_rust_binds_the_new_entries():
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    names = ("pw_execution_blocks_from_pcs", "pw_execution_blocks_from_traces", "pw_execution_blocks_destroy", "pw_execution_blocks_sizes",
             "pw_execution_blocks_read_pc_counts", "pw_execution_blocks_read_runs", "pw_execution_blocks_read_superblocks", "pw_execution_blocks_count",
             "pw_execution_blocks_set_fingerprint_mask", "pw_execution_blocks_last_stats")
    for name in names:
        assert name in c and r.get(name) == c[name], name
    assert c["pw_execution_blocks_from_pcs"] == 10 and c["pw_execution_blocks_from_traces"] == 12
