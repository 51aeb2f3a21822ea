"""Empirical constraints without a GPU: the reference route of tests/_empirical_ref.py on the golden unit case, the
host-side semantics of powdr_amd.empirical.EmpiricalConstraints (combine_with, apply_pc_threshold, the JSON layout), the percentile
positions, and every refusal of pw_empirical_detect that is made before any GPU call."""
import copy
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _empirical_ref as ref

GOLDEN = json.loads((Path(__file__).parent / "golden" / "empirical_unit_case.json").read_text())


def golden_rows(first_ts=10):
    return [(0, 0, first_ts + k, pc, cells) for k, (pc, cells) in enumerate(GOLDEN["rows"])]


def golden_want():
    return dict(column_ranges_by_pc={int(pc): [tuple(r) for r in v] for pc, v in GOLDEN["column_ranges_by_pc"].items()},
                equivalence_classes_by_block={int(b): [[tuple(c) for c in cls] for cls in v] for b, v in GOLDEN["equivalence_classes_by_block"].items()},
                pc_counts={int(pc): n for pc, n in GOLDEN["pc_counts"].items()}, air_id_by_pc={0: 0, 4: 0})


def test_the_reference_route_reproduces_the_golden_case():
    got = ref.detect_rows(golden_rows(), GOLDEN["blocks"], GOLDEN["pc_step"])
    assert got == golden_want()
    assert ref.detect_rows(golden_rows()[::-1], GOLDEN["blocks"], GOLDEN["pc_step"]) == got  # rows in any order: time decides
    # and through the block log AIR: the three cells are columns 3 .. 5 behind [is_valid, pc, ts]
    rows = [(pc, 10 + k, cells) for k, (pc, cells) in enumerate(GOLDEN["rows"])]
    full = ref.detect([(ref.block_log(rows, 3), ref.block_log_interactions())], GOLDEN["blocks"])
    assert {pc: r[3:] for pc, r in full["column_ranges_by_pc"].items()} == got["column_ranges_by_pc"]
    data = [[(i, c - 3) for i, c in cls if c >= 3] for cls in full["equivalence_classes_by_block"][0]]
    assert sorted(c for c in data if len(c) >= 2) == got["equivalence_classes_by_block"][0]


def test_the_reference_route_statuses():
    rows = golden_rows()
    with pytest.raises(ref.Status) as e:
        ref.detect_rows(rows[:3], GOLDEN["blocks"])  # the tail cut off
    assert (e.value.status, e.value.info) == (3, 12)
    with pytest.raises(ref.Status) as e:
        ref.detect_rows(rows + [(0, 0, 11, 8, [0, 0, 0])], GOLDEN["blocks"])
    assert (e.value.status, e.value.info) == (4, 11)
    with pytest.raises(ref.Status) as e:
        ref.detect_rows(rows + [(1, 0, 99, 4, [0, 0, 0])], [])
    assert (e.value.status, e.value.info) == (5, 4)
    with pytest.raises(ref.Status) as e:
        ref.detect_rows(rows[1:], GOLDEN["blocks"])  # pc 4 without its head
    assert (e.value.status, e.value.info) == (3, 11)


def batch_rows():
    """block {0, 2} over 3 columns, four instances: (0,0) = (1,1) in all of them, (0,1) = (1,0) in the first two only, (0,2) = (1,2) in
    the last two only; pc 100 lies in no block"""
    rows, ts = [], 1
    for inst, (a, b0, b1, c0, c1) in enumerate([(5, 7, 7, 1, 2), (6, 8, 8, 3, 4), (7, 9, 1, 5, 5), (8, 2, 3, 6, 6)]):
        rows += [(0, 0, ts, 0, [a, b0, c0]), (0, 0, ts + 1, 4, [b1, a, c1]), (1, 0, ts + 2, 100, [inst, 40 - inst])]
        ts += 3
    return rows


def test_combine_with_follows_the_batch_wise_semantics():
    from powdr_amd import empirical

    rows, blocks = batch_rows(), [(0, 2)]
    first, second = ref.detect_rows(rows[:6], blocks), ref.detect_rows(rows[6:], blocks)
    whole = ref.detect_rows(rows, blocks)
    a, b = ref.to_constraints(first), ref.to_constraints(second)
    assert a.combine_with(b) is a
    got = ref.as_dict(a)
    # ranges: min / max of the per-batch percentiles, pc by pc and column by column
    for pc in (0, 4, 100):
        want = [(min(x[0], y[0]), max(x[1], y[1])) for x, y in zip(first["column_ranges_by_pc"][pc], second["column_ranges_by_pc"][pc])]
        assert got["column_ranges_by_pc"][pc] == want
    assert got["pc_counts"] == whole["pc_counts"] == {0: 4, 4: 4, 100: 4}
    # a class that splits: {(0,1),(1,0)} holds in the first batch, {(0,2),(1,2)} in the second; only {(0,0),(1,1)} in both
    assert first["equivalence_classes_by_block"][0] == [[(0, 0), (1, 1)], [(0, 1), (1, 0)]]
    assert second["equivalence_classes_by_block"][0] == [[(0, 0), (1, 1)], [(0, 2), (1, 2)]]
    assert got["equivalence_classes_by_block"] == whole["equivalence_classes_by_block"] == {0: [[(0, 0), (1, 1)]]}
    # a three-cell class against a two-cell one: the cell missing on one side is a singleton
    assert empirical.intersect_partitions([[(0, 0), (0, 1), (1, 0)]], [[(0, 0), (1, 0)], [(0, 1), (1, 1)]]) == [[(0, 0), (1, 0)]]
    assert empirical.intersect_partitions([[(0, 0), (0, 1)]], []) == []
    # a pc and a block on one side only are kept
    other = empirical.EmpiricalConstraints({8: [(1, 2)]}, {8: [[(0, 0), (0, 1)]]}, {8: 3}, {"air_id_by_pc": {8: 2}, "column_names_by_air_id": {2: ["x", "y"]}})
    a.combine_with(other)
    assert a.column_ranges_by_pc[8] == [(1, 2)] and a.equivalence_classes_by_block[8] == [[(0, 0), (0, 1)]] and a.pc_counts[8] == 3
    assert a.debug_info["air_id_by_pc"] == {0: 0, 4: 0, 100: 1, 8: 2} and a.debug_info["column_names_by_air_id"] == {2: ["x", "y"]}
    # debug maps must agree
    before = copy.deepcopy(a)
    for clash in ({"air_id_by_pc": {4: 1}, "column_names_by_air_id": {}}, {"air_id_by_pc": {}, "column_names_by_air_id": {2: ["x", "z"]}}):
        with pytest.raises(ValueError):
            a.combine_with(empirical.EmpiricalConstraints(debug_info=clash))
    assert a == before


def test_apply_pc_threshold():
    ec = ref.to_constraints(ref.detect_rows(batch_rows(), [(0, 2)]), {0: ["a", "b", "c"], 1: ["n", "m"]})
    same = ec.apply_pc_threshold(1)
    assert same == ec and same is not ec
    for threshold in (100, 4 + 1):
        cut = ec.apply_pc_threshold(threshold)
        assert cut.column_ranges_by_pc == {} and cut.equivalence_classes_by_block == {}
        assert cut.pc_counts == ec.pc_counts and cut.debug_info == ec.debug_info
    assert ec.apply_pc_threshold(4) == ec
    ec.pc_counts[100] = 3
    cut = ec.apply_pc_threshold(4)
    assert sorted(cut.column_ranges_by_pc) == [0, 4] and sorted(cut.equivalence_classes_by_block) == [0] and cut.pc_counts[100] == 3
    assert ec.apply_pc_threshold().column_ranges_by_pc == {}  # the default is the reference's 100


def test_json_layout():
    from powdr_amd import empirical

    ec = ref.to_constraints(ref.detect_rows(golden_rows(), GOLDEN["blocks"]), {0: GOLDEN["column_names"]})
    text = ec.to_json()
    assert text == "\n".join(GOLDEN["document_lines"])
    assert list(json.loads(text)) == ["column_ranges_by_pc", "equivalence_classes_by_block", "debug_info", "pc_counts"]
    assert empirical.EmpiricalConstraints.from_json(text) == ec
    big = ref.to_constraints(ref.detect_rows(batch_rows(), [(0, 2)]), {1: ["n", "m"]})
    back = empirical.EmpiricalConstraints.from_json(big.to_json())
    assert back == big and back.to_json() == big.to_json()
    assert list(json.loads(big.to_json())["pc_counts"]) == ["0", "4", "100"]  # numeric order, not the order of the strings


@pytest.mark.parametrize("n", [1, 2, 99, 100, 101, 199, 200, 2**32 - 1])
def test_percentile_indices(n):
    from powdr_amd import empirical

    assert empirical.percentile_indices(n) == (n // 100, n * 99 // 100) == ref.percentile_indices(n)


def test_refusals_before_any_gpu_call():
    from powdr_amd import empirical, prover

    lib = empirical.lib
    none = (prover.PwSegmentAir * 1)()
    blocks = lambda *b: (empirical.PwBasicBlock * max(len(b), 1))(*[empirical.PwBasicBlock(s, n) for s, n in b])
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    call = lambda airs, n_airs, pc_step, blk, n_blk, o=C.byref(out), s=C.byref(status), i=C.byref(info): lib.pw_empirical_detect(
        airs, None, n_airs, 0, pc_step, blk, n_blk, 0, o, s, i)
    # no AIRs: an empty result, no GPU needed
    assert call(none, 0, 4, blocks((0, 2)), 1) == 0 and status.value == 0 and out.value
    sizes = (C.c_uint64 * 5)()
    lib.pw_empirical_sizes(out, sizes)
    assert list(sizes) == [0, 0, 0, 0, 0]
    lib.pw_empirical_destroy(out)
    assert call(None, 0, 4, None, 0) == 0 and out.value  # no AIRs, no blocks
    lib.pw_empirical_destroy(out)
    # NULL pointers
    assert call(None, 1, 4, blocks(), 0) == -1
    assert call(none, 0, 4, None, 1) == -1
    assert call(none, 0, 4, blocks(), 0, o=None) == -1
    assert call(none, 0, 4, blocks(), 0, s=None) == -1
    assert call(none, 0, 4, blocks(), 0, i=None) == -1
    assert call(none, 1, 4, blocks(), 0) == -1  # an entry without a prover
    none[0] = prover.PwSegmentAir(None, 16, 3, 0)
    assert call(none, 1, 4, blocks(), 0) == -1
    # pc_step 0; block tables: a zero count, unsorted, equal starts, overlapping, past 2^32
    assert call(none, 0, 0, blocks((0, 2)), 1) == -1
    for bad in ([(0, 0)], [(8, 1), (0, 1)], [(8, 1), (8, 1)], [(0, 3), (8, 1)], [(0xFFFFFFFC, 2)]):
        assert call(none, 0, 4, blocks(*bad), len(bad)) == -1, bad
    for good in ([(0, 2), (8, 1)], [(0xFFFFFFF8, 2)], [(0, 1), (4, 1), (8, 5)]):
        assert call(none, 0, 4, blocks(*good), len(good)) == 0, good
        lib.pw_empirical_destroy(out)
    with pytest.raises(Exception):
        empirical.detect([], [(0, 2)], pc_step=0)
    assert empirical.detect([], [(0, 2)]) == empirical.EmpiricalConstraints()


def test_rust_binds_the_new_entries():
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name in ("pw_empirical_detect", "pw_empirical_destroy", "pw_empirical_sizes", "pw_empirical_read_pcs", "pw_empirical_read_ranges",
                 "pw_empirical_read_blocks", "pw_empirical_read_cells", "pw_empirical_percentile_indices", "pw_empirical_set_fingerprint_mask",
                 "pw_empirical_last_stats"):
        assert name in c and r.get(name) == c[name]
    assert c["pw_empirical_detect"] == 11
