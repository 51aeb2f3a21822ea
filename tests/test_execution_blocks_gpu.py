"""pw_execution_blocks_from_pcs / _from_traces / _count on the GPU against the second route of
tests/_execution_blocks_ref.py: every field, exactly, in the map's order."""
import json
from pathlib import Path

import numpy as np
import pytest

from tests import _empirical_ref as eref
from tests import _execution_blocks_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = json.loads((Path(__file__).parent / "golden" / "execution_blocks_unit_cases.json").read_text())
IT = eref.block_log_interactions()
A, B, C3, D = 0x100, 0x200, 0x300, 0x400   # blocks of 2, 3, 2 and 4 instructions
S1, S2 = 0x800, 0x900                      # one-instruction blocks
BLOCKS = [(A, 2), (B, 3), (C3, 2), (D, 4), (S1, 1), (S2, 1)]
SIZES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1025, 2**16 + 1]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def expand(heads, blocks=BLOCKS, pc_step=4):
    """the pcs of a sequence of block heads"""
    n = dict(blocks)
    return [h + k * pc_step for h in heads for k in range(n[h])]


def check(gpu, pcs, blocks=BLOCKS, max_bb=1, pc_step=4, **kw):
    """the device result of a pc list, compared field by field (and key order by key order) with the second route; the caller closes"""
    from powdr_amd import execution_blocks as eb

    want = ref.detect(pcs, blocks, max_bb=max_bb, pc_step=pc_step)
    got = eb.detect(pcs, blocks, max_bb=max_bb, pc_step=pc_step, **kw)
    assert got.pc_count == want["pc_count"] and list(got.pc_count) == list(want["pc_count"])
    assert got.execution_bb_runs == want["execution_bb_runs"]
    assert got.superblock_counts == want["superblock_counts"] and list(got.superblock_counts) == list(want["superblock_counts"])
    got.want = want
    return got


def status_of(gpu, pcs, blocks=BLOCKS, max_bb=1, **kw):
    from powdr_amd import execution_blocks as eb

    with pytest.raises(eb.ExecutionBlocksError) as e:
        eb.detect(pcs, blocks, max_bb=max_bb, **kw)
    with pytest.raises(ref.Status) as want:
        ref.detect(pcs, blocks, max_bb=max_bb)
    assert (e.value.status, e.value.info) == (want.value.status, want.value.info)
    assert eb.last_stats()["scratch_bytes"] == 0  # (a status raised after the heads stage allocated)
    return e.value.status, e.value.info


# ---- the reference's unit cases ---------------------------------------------------------------------------------------------------------
def test_the_golden_detect_superblocks_case(gpu):
    g = GOLDEN["detect_superblocks"]
    with check(gpu, g["execution"], g["blocks"], max_bb=g["max_bb"], pc_step=g["pc_step"]) as got:
        assert got.execution_bb_runs == [(tuple(r["start_pcs"]), r["count"]) for r in g["execution_bb_runs"]]
        for c in g["counts"]:
            assert got.superblock_counts[tuple(c["start_pcs"])] == c["count"]
        assert all(tuple(a) not in got.superblock_counts for a in g["absent"])
        assert got.blocks(exec_count_cutoff=2) == [((100,), 2), ((100, 200), 2), ((200,), 2)]
        assert got.blocks(max_instructions=3) == [((100,), 2), ((200,), 2), ((400,), 1)]


def golden_run(values):
    """a run of the golden cases' small numbers as two-instruction blocks at 16 * value"""
    blocks = [(16 * v, 2) for v in range(1, 7)]
    return expand([16 * v for v in values], blocks), blocks


def test_the_golden_run_cases(gpu):
    g = GOLDEN["superblocks_in_run"]
    pcs, blocks = golden_run(g["run"])
    with check(gpu, pcs, blocks, max_bb=g["max_len"]) as got:
        assert len(got.superblock_counts) == g["n_superblocks"]
        for c in g["counts"]:
            assert got.superblock_counts[tuple(16 * v for v in c["start_pcs"])] == c["count"]
    for case in GOLDEN["find_non_overlapping"]:
        pcs, blocks = golden_run(case["haystack"])
        with check(gpu, pcs, blocks, max_bb=3) as got:
            assert got.count([16 * v for v in case["needle"]]) == len(case["indices"])
    for case in GOLDEN["count_and_update_run"]:
        pcs, blocks = golden_run(case["run"])
        with check(gpu, pcs, blocks, max_bb=3) as got:
            assert got.count([16 * v for v in case["needle"]], remove=True) == case["count"]
            for L in (1, 2, 3):  # what is left answers every window of the run as the reference's sub-runs do
                for i in range(len(case["run"]) - L + 1):
                    w = case["run"][i:i + L]
                    assert got.count([16 * v for v in w]) == ref.count(w, case["sub_runs"]), (case, w)


# ---- self-overlap: greedy chains across waves and workgroups -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_one_block_repeated(gpu, n):
    from powdr_amd import execution_blocks as eb

    with check(gpu, expand([A] * n), max_bb=3) as got:
        want = {(A,): n}
        if n >= 2:
            want[(A, A)] = n // 2
        if n >= 3:
            want[(A, A, A)] = n // 3
        assert got.superblock_counts == want and got.execution_bb_runs == [((A,) * n, 1)]
        stats = eb.last_stats()
        assert stats["levels"] == min(n, 3) and stats["heads"] == stats["runs"] * n == n
        assert stats["jumping_clusters"] == (n >= 3) + (n >= 4)  # one cluster per self-overlapping window


@pytest.mark.parametrize("n", SIZES)
def test_period_two_and_three(gpu, n):
    for period in ([A, B], [A, B, C3]):
        run = (period * (n // len(period) + 1))[:n]
        with check(gpu, expand(run), max_bb=4) as got:
            if n >= 4 and len(period) == 2:
                assert got.superblock_counts[(A, B, A)] == len(ref.find_non_overlapping(run, [A, B, A])) == (n + 1) // 4
                assert got.superblock_counts[(A, B, A, B)] == n // 4
            if n >= 4 and len(period) == 3:
                assert got.superblock_counts[(A, B, C3, A)] == len(ref.find_non_overlapping(run, [A, B, C3, A]))


def test_the_overlap_of_the_unit_test(gpu):
    from powdr_amd import execution_blocks as eb

    torch, _ = gpu
    pcs = expand([A, B, A, B, A])
    with check(gpu, pcs, max_bb=3) as got:
        assert got.superblock_counts[(A, B, A)] == 1 and got.superblock_counts[(A, B)] == 2 and got.superblock_counts[(B, A)] == 2
        # the pcs as a tensor that is on the device already: read in place
        with eb.detect(torch.tensor(pcs, dtype=torch.int32, device="cuda"), BLOCKS, max_bb=3) as same:
            assert same.superblock_counts == got.superblock_counts and same.execution_bb_runs == got.execution_bb_runs
    with pytest.raises(ValueError):
        eb.detect(torch.tensor(pcs, dtype=torch.int64, device="cuda"), BLOCKS)


# ---- windows and cuts ------------------------------------------------------------------------------------------------------------------
def test_windows_do_not_cross_a_cut(gpu):
    with check(gpu, expand([A, B, S1, A, B]), max_bb=2) as got:
        assert (B, A) not in got.superblock_counts and got.superblock_counts[(A, B)] == 2
        assert got.execution_bb_runs == [((A, B), 2)] and got.pc_count[S1] == 1
        assert got.count([B, A]) == 0


def test_max_bb_against_the_run_lengths(gpu):
    from powdr_amd import execution_blocks as eb

    heads = [A, B, C3, S1, D, S2, S1, B, A, S2]
    with check(gpu, expand(heads), max_bb=7) as got:  # above every run length: the levels stop at 3
        assert eb.last_stats()["levels"] == 3 and max(len(w) for w in got.superblock_counts) == 3
    with check(gpu, expand(heads), max_bb=255):
        assert eb.last_stats()["levels"] == 3
    with check(gpu, expand(heads), max_bb=1) as got:
        assert set(got.superblock_counts) == {(A,), (B,), (C3,), (D,)} and eb.last_stats()["levels"] == 1
    with check(gpu, expand([A] * 300), max_bb=255) as got:  # every length up to 255 on one run
        assert len(got.superblock_counts) == 255 and got.superblock_counts[(A,) * 255] == 1 and got.superblock_counts[(A,) * 150] == 2


def test_no_runs_and_no_pcs(gpu):
    from powdr_amd import execution_blocks as eb

    with check(gpu, expand([S1, S2, S2, S1]), max_bb=3) as got:
        assert got.execution_bb_runs == [] and got.superblock_counts == {} and got.pc_count == {S1: 2, S2: 2}
        assert got.count([S1]) == 0 and got.resident_heads == 0 and eb.last_stats()["runs"] == 0
    with check(gpu, [], max_bb=3) as got:
        assert got.pc_count == {} and got.execution_bb_runs == [] and got.superblock_counts == {}


# ---- runs ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("times", [1, 2, 1000])
def test_one_run_many_times(gpu, times):
    run = [A, B, B, D, A]
    with check(gpu, expand((run + [S1]) * times), max_bb=3) as got:
        assert got.execution_bb_runs == [(tuple(run), times)] and got.superblock_counts[(B, D, A)] == times
        assert got.count([B, B]) == times


def test_runs_that_differ_in_one_place(gpu):
    base = [A, B, C3, D, A, B]
    runs = [base, base[:-1] + [D], [D] + base[1:], base[:-1], base + [A], base, base[:-1]]
    heads = [h for r in runs for h in r + [S2]]
    with check(gpu, expand(heads), max_bb=4) as got:
        assert len(got.execution_bb_runs) == 5 and dict(got.execution_bb_runs)[tuple(base)] == 2 and dict(got.execution_bb_runs)[tuple(base[:-1])] == 2
        keys = [r for r, _ in got.execution_bb_runs]
        assert keys.index(tuple(base[:-1])) + 1 == keys.index(tuple(base)) and keys.index(tuple(base)) + 1 == keys.index(tuple(base + [A]))


def test_4096_distinct_runs(gpu):
    from powdr_amd import execution_blocks as eb

    heads = []
    for v in np.random.default_rng(2).permutation(1 << 12).tolist():
        heads += [A if (v >> k) & 1 else B for k in range(12)] + [S1]
    with check(gpu, expand(heads), max_bb=3) as got:
        assert len(got.execution_bb_runs) == 1 << 12 and set(c for _, c in got.execution_bb_runs) == {1}
        assert len(got.superblock_counts) == 2 + 4 + 8 and eb.last_stats()["seeds"] == 1 and eb.last_stats()["runs"] == 1 << 12


def test_masked_fingerprints_stay_exact(gpu):
    from powdr_amd import execution_blocks as eb

    rng = np.random.default_rng(7)
    heads = []
    for _ in range(300):
        heads += [[A, B, C3, D][i] for i in rng.integers(0, 4, size=int(rng.integers(1, 4)))] + [S1]
    same = expand(([A, B, D] + [S2]) * 50)
    try:
        for mask in (0x7, 0xFF):
            eb.set_fingerprint_mask(mask)
            try:
                check(gpu, expand(heads), max_bb=3).close()  # exact
            except eb.ExecutionBlocksError as e:
                assert e.status == 6  # or refused, never wrong
            assert eb.last_stats()["seeds"] in (1, 2, 3)
        eb.set_fingerprint_mask(1)
        with check(gpu, same, max_bb=2) as got:  # equal runs collide under any mask and verify
            assert got.execution_bb_runs == [((A, B, D), 50)] and eb.last_stats()["seeds"] == 1
    finally:
        eb.set_fingerprint_mask(0)
    check(gpu, expand(heads), max_bb=3).close()
    assert eb.last_stats()["seeds"] == 1


# ---- structure and scratch ---------------------------------------------------------------------------------------------------------------
def test_a_last_block_cut_off_counts(gpu):
    with check(gpu, expand([A, D, S1, B, D])[:-2], max_bb=2) as got:
        assert got.superblock_counts[(D,)] == 2 and got.superblock_counts[(B, D)] == 1 and got.pc_count[D] == got.pc_count[D + 4] == 2 and got.pc_count[D + 8] == 1
    with check(gpu, [B], max_bb=2) as got:
        assert got.superblock_counts == {(B,): 1}


def test_status_3_names_the_first_offence(gpu):
    good = expand([A, B, S1, D, A])
    assert status_of(gpu, good[1:]) == (3, 0)                                  # the first pc is no start
    assert status_of(gpu, good[:5] + [0x7000] + good[5:]) == (3, 5)            # a pc in no block, where a head must be
    assert status_of(gpu, good[:3] + [B + 8] + good[4:]) == (3, 3)             # an in-block pc that does not follow
    assert status_of(gpu, good[:6] + [D + 8] + good[7:-1] + [A]) == (3, 6)     # two offences: the smallest
    assert status_of(gpu, good[:3] + good[4:]) == (3, 3)                       # an instruction missing: the next one does not follow
    assert status_of(gpu, good[:2] + good[3:]) == (3, 2)                       # a head missing: its second instruction is no start
    assert status_of(gpu, [A, A + 4] * 40000 + [A + 4]) == (3, 80000)          # far from the start
    assert status_of(gpu, good, blocks=[]) == (3, 0)


def test_status_2_and_the_bytes_it_names(gpu):
    from powdr_amd import execution_blocks as eb

    pcs = expand(([A, B, A, B, D] + [S1]) * 40)
    with pytest.raises(eb.ExecutionBlocksError) as e:
        eb.detect(pcs, BLOCKS, max_bb=3, scratch_bytes=1)
    assert e.value.status == 2 and e.value.info > 1 and eb.last_stats()["scratch_bytes"] == 0
    with check(gpu, pcs, max_bb=3, scratch_bytes=e.value.info) as got:
        stats = eb.last_stats()
        assert stats["peak_bytes"] <= e.value.info and stats["scratch_bytes"] == 0 and got.resident_heads == 200
    with pytest.raises(eb.ExecutionBlocksError) as again:
        eb.detect(pcs, BLOCKS, max_bb=3, scratch_bytes=e.value.info // 16)
    assert again.value.status == 2 and eb.last_stats()["scratch_bytes"] == 0  # (refused at the levels: the heads stage had its buffers)


# ---- count / remove on the resident execution -------------------------------------------------------------------------------------------
def test_candidates_counted_and_removed_in_order(gpu):
    rng = np.random.default_rng(11)
    heads = []
    for _ in range(200):
        heads += [[A, B, C3][i] for i in rng.integers(0, 3, size=int(rng.integers(1, 9)))] + [S1]
    heads += [A] * 700 + [S2] + [A, B] * 300
    from powdr_amd import execution_blocks as eb

    with check(gpu, expand(heads), max_bb=2) as got:
        runs = got.want["runs"]
        peak = eb.last_stats()["peak_bytes"]
        steps = [([A, B], False), ([A, A], True), ([A, A, A], False), ([A, B], True), ([B, A], True), ([A, B], False), ([0x7000], True),
                 ([C3, A, 0x7000], False), ([A], True), ([B, C3], False), ([A] * 400, False), ([C3, C3], True), ([C3], True)]
        seen = []
        for needle, remove in steps:
            if remove:
                want, runs = ref.count_and_update_execution(needle, runs)
            else:
                want = ref.count(needle, runs)
            assert got.count(needle, remove=remove) == want, (needle, remove)
            seen.append(want)
            # a count releases what it took; the detection's peak stands unless the count held more: at most 40 bytes per resident head
            # (flags, positions, five arrays per match) and a scan's temporary storage, which is less than a level's 168 per head
            stats = eb.last_stats()
            assert stats["scratch_bytes"] == 0 and peak <= stats["peak_bytes"] <= max(peak, 65536 + 168 * len(heads))
        assert seen[0] > 300 and seen[1] >= 350 and seen[5] == 0 and seen[6] == 0 and seen[10] == 0  # [A, B] no longer occurs after its removal
        assert got.count([B]) == ref.count([B], runs) > 0


# ---- the trace route ----------------------------------------------------------------------------------------------------------------------
def traces_of(gpu, logs, blocks, max_bb, segments=None, **kw):
    from powdr_amd import execution_blocks as eb
    from tests.test_bus_check_gpu import Segment

    s = Segment(gpu, logs)
    try:
        return eb.detect(s.seg, blocks, max_bb=max_bb, segments=segments, **kw)
    finally:
        s.close()


def test_traces_in_any_row_order_equal_the_pc_list(gpu):
    rng = np.random.default_rng(3)
    heads = []
    for _ in range(60):
        heads += [[A, B, C3, D][i] for i in rng.integers(0, 4, size=int(rng.integers(1, 7)))] + [S1 if rng.integers(0, 2) else S2]
    pcs = expand(heads)
    half = len(pcs) // 2
    # rows alternate between two AIRs of segment 0, a third AIR holds segment 1 with timestamps that start again; every AIR permuted, with padding
    rows = [[], [], []]
    for t, pc in enumerate(pcs[:half]):
        rows[t % 2].append((pc, 100 + t, [t]))
    for t, pc in enumerate(pcs[half:]):
        rows[2].append((pc, 5 + t, [t]))
    logs = [(eref.block_log(r, 1, log_h=10, places=rng.permutation(1 << 10)[:len(r)]), IT) for r in rows]
    with check(gpu, pcs, max_bb=3) as want, traces_of(gpu, logs, BLOCKS, 3, segments=[0, 0, 1]) as got:
        assert got.pc_count == want.pc_count and got.execution_bb_runs == want.execution_bb_runs
        assert got.superblock_counts == want.superblock_counts and list(got.superblock_counts) == list(want.superblock_counts)
        assert got.count([A, B], remove=True) == want.count([A, B], remove=True) and got.count([B]) == want.count([B])


def test_trace_statuses(gpu):
    from powdr_amd import execution_blocks as eb

    pcs = expand([A, B, S1, A])
    rows = [(pc, 10 + t, [0]) for t, pc in enumerate(pcs)]
    log = lambda rs: [(eref.block_log(rs, 1), IT)]
    traces_of(gpu, log(rows), BLOCKS, 2).close()
    with pytest.raises(eb.ExecutionBlocksError) as e:  # 3: the time key of the offending row, not its position
        traces_of(gpu, log(rows[:3] + [(B + 8, 13, [0])] + rows[4:]), BLOCKS, 2, segments=[2])
    assert (e.value.status, e.value.info) == (3, (2 << 32) | 13) and eb.last_stats()["scratch_bytes"] == 0
    with pytest.raises(eb.ExecutionBlocksError) as e:  # 4: a duplicate time key
        traces_of(gpu, log(rows + [(S1, 12, [0])]), BLOCKS, 2)
    assert (e.value.status, e.value.info) == (4, 12) and eb.last_stats()["scratch_bytes"] == 0
    twice = eref.block_log(rows, 1)
    twice[0, 3] = 2
    with pytest.raises(eb.ExecutionBlocksError) as e:  # 7: a multiplicity of 2, the smallest (air, row)
        traces_of(gpu, log(rows) + [(twice, IT)], BLOCKS, 2)
    assert (e.value.status, e.value.info) == (7, (1 << 32) | 3) and eb.last_stats()["scratch_bytes"] == 0
    with pytest.raises(eb.ExecutionBlocksError) as e:
        traces_of(gpu, log(rows), BLOCKS, 2, scratch_bytes=1)
    assert e.value.status == 2 and e.value.info > 1
    with traces_of(gpu, log(rows), BLOCKS, 2, scratch_bytes=e.value.info) as got:
        assert got.execution_bb_runs == [((A,), 1), ((A, B), 1)] and eb.last_stats()["peak_bytes"] <= e.value.info
    with traces_of(gpu, log(rows), BLOCKS, 2, bus=1) as got:  # no AIR on the bus: an empty execution
        assert got.pc_count == {}


def test_the_chained_execution(gpu):
    from powdr_amd import execution_blocks as eb
    from tests import _chained_vm as vm
    from tests.test_empirical_gpu import device_airs

    ex = vm.Execution(64, seed=3)
    blocks = [(vm.START_PC, len(vm.BLOCK))]
    pcs = [vm.START_PC + 4 * i for i in range(len(vm.BLOCK))] * 64  # the executor's path: the block, 64 times
    seg, keep, _ = device_airs(gpu, ex.table, ex.rec, 64)
    try:
        with check(gpu, pcs, blocks, max_bb=3) as want, eb.detect(seg, blocks, max_bb=3) as got:
            assert got.pc_count == want.pc_count == {pc: 64 for pc in pcs[:len(vm.BLOCK)]}
            assert got.execution_bb_runs == want.execution_bb_runs == [((vm.START_PC,) * 64, 1)]
            assert got.superblock_counts == want.superblock_counts == {(vm.START_PC,): 64, (vm.START_PC,) * 2: 32, (vm.START_PC,) * 3: 21}
            assert got.count([vm.START_PC] * 5, remove=True) == 12 and got.count([vm.START_PC] * 4) == 1
    finally:
        for p, _, _ in seg:
            p.close()
