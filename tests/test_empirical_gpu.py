"""pw_empirical_detect on the GPU against the reference route of tests/_empirical_ref.py: every field, exactly."""
import json
from pathlib import Path

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _empirical_ref as ref
from tests.test_bus_check_gpu import Segment

pytestmark = pytest.mark.gpu
P = om.P
GOLDEN = json.loads((Path(__file__).parent / "golden" / "empirical_unit_case.json").read_text())
IT = ref.block_log_interactions()
# both sides of 2^27 and of 2^31 - 2^27 (= p - 1), 0, 1: as Montgomery words x * 2^32 mod p these sort differently
EDGES = [0, 1, P - 1, P - 2, (1 << 27) - 1, 1 << 27, (1 << 27) + 1, (1 << 31) - (1 << 27) - 1]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def run(gpu, host, blocks, segments=None, **kw):
    """the device result of the host AIRs [(cols, interactions)], compared with the reference route"""
    from powdr_amd import empirical

    s = Segment(gpu, host)
    try:
        got = empirical.detect(s.seg, blocks, segments=segments, **kw)
    finally:
        s.close()
    assert ref.as_dict(got) == ref.detect(host, blocks, segments=segments)
    return got


def status_of(gpu, host, blocks, segments=None, **kw):
    """(status, info) of a call that must fail, on the device and by the reference route; no result object exists"""
    from powdr_amd import empirical, stage

    s = Segment(gpu, host)
    try:
        with pytest.raises(empirical.EmpiricalError) as e:
            empirical.detect(s.seg, blocks, segments=segments, **kw)
        recs, _ = stage.air_records(s.seg)
        blk = (empirical.PwBasicBlock * max(len(blocks), 1))(*[empirical.PwBasicBlock(a, b) for a, b in blocks])
        rc, status, info, handle = stage.raw(empirical.lib.pw_empirical_detect, recs, None, len(s.seg), 0, 4, blk, len(blocks), 0)
        if segments is None:
            assert (rc, status, info, handle) == (0, e.value.status, e.value.info, None)
    finally:
        s.close()
    with pytest.raises(ref.Status) as want:
        ref.detect(host, blocks, segments=segments)
    assert (e.value.status, e.value.info) == (want.value.status, want.value.info)
    assert empirical.last_stats()["scratch_bytes"] < 64 << 10  # (a status raised after the stages allocated: only `small` stays)
    return e.value.status, e.value.info


def data_part(ec, first=3):
    """ranges and classes of the data columns behind [is_valid, pc, ts]"""
    ranges = {pc: r[first:] for pc, r in ec.column_ranges_by_pc.items()}
    classes = {}
    for b, cl in ec.equivalence_classes_by_block.items():
        cut = [[(i, c - first) for i, c in cls if c >= first] for cls in cl]
        classes[b] = sorted(c for c in cut if len(c) >= 2)
    return ranges, classes


def test_the_golden_case(gpu):
    rows = [(pc, 10 + k, cells) for k, (pc, cells) in enumerate(GOLDEN["rows"])]
    got = run(gpu, [(ref.block_log(rows, 3), IT)], GOLDEN["blocks"])
    ranges, classes = data_part(got)
    assert ranges == {int(pc): [tuple(r) for r in v] for pc, v in GOLDEN["column_ranges_by_pc"].items()}
    assert classes == {int(b): [[tuple(c) for c in cls] for cls in v] for b, v in GOLDEN["equivalence_classes_by_block"].items()}
    assert got.pc_counts == {0: 2, 4: 2} and got.debug_info["air_id_by_pc"] == {0: 0, 4: 0}


def test_all_64_traces_of_a_two_instruction_block(gpu):
    """instruction 0 has two data cells (AIR 0), instruction 1 one (AIR 1), two instances, values in {0, 1}: 2^6 traces as 64 blocks"""
    first, second, blocks, ts = [], [], [], 1
    for t in range(64):
        bit = lambda k: (t >> k) & 1
        blocks.append((32 * t, 2))
        for inst in range(2):
            first.append((32 * t, ts, [bit(3 * inst), bit(3 * inst + 1)]))
            second.append((32 * t + 4, ts + 1, [bit(3 * inst + 2)]))
            ts += 2
    got = run(gpu, [(ref.block_log(first, 2), IT), (ref.block_log(second, 1), IT)], blocks)
    _, classes = data_part(got)
    seen = {tuple(map(tuple, cl)) for cl in classes.values()}
    a, b, c = (0, 0), (0, 1), (1, 0)
    assert seen == {(), ((a, b),), ((a, c),), ((b, c),), ((a, b, c),)}  # every partition of three cells
    assert len(got.equivalence_classes_by_block) == 64 and set(got.pc_counts.values()) == {2}


def test_percentile_edges(gpu):
    rng = np.random.default_rng(5)
    rows, ts = [], 1
    for k, n in enumerate([1, 99, 100, 101, 199, 200, 10000]):
        for _ in range(n):
            rows.append((0x100 + 4 * k, ts, [int(rng.choice(EDGES)), int(rng.integers(0, P)), int(rng.choice(EDGES[:4]))]))
            ts += 1
    order = rng.permutation(len(rows))
    got = run(gpu, [(ref.block_log([rows[i] for i in order], 3), IT)], [])
    assert got.pc_counts == {0x100 + 4 * k: n for k, n in enumerate([1, 99, 100, 101, 199, 200, 10000])}
    assert got.equivalence_classes_by_block == {}
    # the order is the canonical one: the Montgomery words of the edge values sort differently
    mont = [int(x) for x in om.to_monty(np.array(sorted(EDGES), np.uint32))]
    assert mont != sorted(mont)
    lo, hi = got.column_ranges_by_pc[0x100 + 4 * 6][3]
    assert lo == 0 and hi == P - 1  # 10 000 draws from eight values: the 1st percentile is the smallest, the 99th the largest


def class_edge_airs(instances_of, seed=3):
    """blocks of three instructions over three AIRs of widths 3, 20 and 61: per block and instance six random source words, cell c of
    an instruction = source (c mod 6) — except, in AIR 1, data cell 7, which leaves its class in the LAST instance only, and data
    cell 8, which leaves it in the FIRST only. Instances of the blocks interleave in time."""
    rng = np.random.default_rng(seed)
    logs, ts = ([], [], []), 1
    todo = [(start, j, n) for start, n in instances_of.items() for j in range(n)]
    order = sorted(range(len(todo)), key=lambda i: (todo[i][1], todo[i][0]))  # round robin over the blocks
    for i in order:
        start, j, n = todo[i]
        src = rng.integers(0, P, size=6).tolist()
        for k, n_data in enumerate((0, 17, 58)):
            data = [src[c % 6] for c in range(n_data)]
            if k == 1:
                if j == n - 1:
                    data[7] = (data[7] + 1) % P
                if j == 0:
                    data[8] = (data[8] + 5) % P
            logs[k].append((start + 4 * k, ts, data))
            ts += 1
    return logs


def test_class_edges(gpu):
    """65, 257 and 1 025 instances (past a wave, a workgroup, a verification tile), a block seen once, a listed one-instruction block,
    pcs in no block, a listed block that never runs, three AIRs of widths 3, 20 and 61 inside one block"""
    counts = {0x1000: 65, 0x2000: 257, 0x3000: 1025, 0x4000: 1}
    logs = class_edge_airs(counts)
    ts = 1 << 20
    for j in range(70):  # a one-instruction block (pc 0x5000, AIR 1): data 0 = data 1 always, data 2 = data 0 but once
        v = 1000 + j
        logs[1].append((0x5000, ts, [v, v, v + (j == 33)] + [j] * 14))
        logs[2].append((0x6000 + 4 * (j % 3), ts + 1, [j % 2] * 58))  # pcs in no block
        ts += 2
    blocks = [(s, 3) for s in counts] + [(0x5000, 1), (0x7000, 4)]
    host = [(ref.block_log(rows, n), IT) for rows, n in zip(logs, (0, 17, 58))]
    got = run(gpu, host, sorted(blocks))
    from powdr_amd import empirical

    stats = empirical.last_stats()
    assert stats["seeds"] == 1 and stats["cells_verified"] > 0 and stats["scratch_bytes"] < 64 << 10 < stats["peak_bytes"]
    assert sorted(got.equivalence_classes_by_block) == [0x1000, 0x2000, 0x3000, 0x4000, 0x5000]
    for start, n in counts.items():
        cl = got.equivalence_classes_by_block[start]
        where = lambda cell: next((k for k, c in enumerate(cl) if cell in c), None)
        # data cell d of AIR 1 is column 3 + d of instruction 1; source 1 is also data cell 1
        together = lambda d: where((1, 3 + d)) is not None and where((1, 3 + d)) == where((1, 3 + d % 6))
        assert together(13) and together(9)
        assert not together(7) and not together(8)  # they left in one instance only (seen once: in that one)
    one = got.equivalence_classes_by_block[0x5000]
    assert any((0, 3) in c and (0, 4) in c and (0, 5) not in c for c in one)
    assert got.pc_counts[0x6000] == 24 and 0x7000 not in got.pc_counts
    assert got.debug_info["air_id_by_pc"][0x1000] == 0 and got.debug_info["air_id_by_pc"][0x1004] == 1 and got.debug_info["air_id_by_pc"][0x1008] == 2
    assert [len(got.column_ranges_by_pc[0x1000 + 4 * k]) for k in range(3)] == [3, 20, 61]


def test_order_and_padding_do_not_change_a_byte(gpu):
    counts = {0x1000: 130, 0x2000: 3}
    logs = class_edge_airs(counts, seed=8)
    blocks = [(s, 3) for s in counts]
    plain = run(gpu, [(ref.block_log(rows, n), IT) for rows, n in zip(logs, (0, 17, 58))], blocks)
    again = run(gpu, [(ref.block_log(rows, n), IT) for rows, n in zip(logs, (0, 17, 58))], blocks)
    rng = np.random.default_rng(1)
    moved = [(ref.block_log(rows, n, log_h=10, places=rng.permutation(1 << 10)[:len(rows)]), IT) for rows, n in zip(logs, (0, 17, 58))]
    shuffled = run(gpu, moved, blocks)
    assert plain == again == shuffled and plain.to_json() == again.to_json() == shuffled.to_json()
    # a padding row's zeros leak into no range: every is_valid range is (1, 1)
    assert all(r[0] == (1, 1) for r in shuffled.column_ranges_by_pc.values())


def test_segments_order_the_time_keys(gpu):
    """one instance of block {0, 2}: its head in an AIR entry of segment 0 at timestamp 1000, its second row in an entry of segment 1
    at timestamp 5 — segment << 32 | timestamp puts the head first; without the segments the second row comes first (status 3)"""
    a = ref.block_log([(0x40, 999, [1, 2]), (0, 1000, [7, 7])], 2)
    b = ref.block_log([(4, 5, [7, 8]), (0x44, 6, [3, 3])], 2)
    got = run(gpu, [(a, IT), (b, IT)], [(0, 2)], segments=[0, 1])
    assert got.pc_counts == {0: 1, 4: 1, 0x40: 1, 0x44: 1}
    assert [(0, 3), (0, 4), (1, 3)] in got.equivalence_classes_by_block[0]
    assert status_of(gpu, [(a, IT), (b, IT)], [(0, 2)]) == (3, 5)


def test_panels_within_a_scratch_bound(gpu):
    from powdr_amd import empirical

    counts = {0x1000: 40, 0x2000: 2}
    logs = class_edge_airs(counts, seed=4)
    blocks = [(s, 3) for s in counts]
    host = [(ref.block_log(rows, n, log_h=6), IT) for rows, n in zip(logs, (0, 17, 58))]
    whole = run(gpu, host, blocks)
    assert empirical.last_stats()["panels"] == 1
    s = Segment(gpu, host)
    try:
        with pytest.raises(empirical.EmpiricalError) as e:
            empirical.detect(s.seg, blocks, scratch_bytes=1)  # below one column
        assert e.value.status == 2 and e.value.info > 1 and empirical.last_stats()["scratch_bytes"] < 64 << 10
        bound = e.value.info
        for _ in range(2):  # (the first figure is what is known before a row is read; a second one is exact)
            try:
                tight = empirical.detect(s.seg, blocks, scratch_bytes=bound)
                break
            except empirical.EmpiricalError as again:
                assert again.status == 2 and again.info > bound
                bound = again.info
        stats = empirical.last_stats()
        assert stats["panels"] >= 3 and stats["peak_bytes"] <= bound
        assert tight == whole and tight.to_json() == whole.to_json()
    finally:
        s.close()


def test_statuses_with_their_info(gpu):
    from powdr_amd import abi, empirical, periphery

    rows = [(0, 10, [1]), (4, 11, [2]), (8, 12, [3]), (0, 20, [1]), (4, 21, [2]), (8, 22, [3])]
    blocks = [(0, 3)]
    log = lambda rs: [(ref.block_log(rs, 1), IT)]
    run(gpu, log(rows), blocks)
    assert status_of(gpu, log(rows[:5]), blocks) == (3, 20)                       # a tail cut off
    assert status_of(gpu, log(rows[:4] + [(12, 21, [2])] + rows[5:]), blocks) == (3, 20)  # the chain broken in the middle
    assert status_of(gpu, log(rows[:1] + rows[2:]), blocks) == (3, 10)
    assert status_of(gpu, log(rows + [(0x40, 21, [9])]), blocks) == (4, 21)        # a duplicate time key
    other = ref.block_log([(4, 30, [5, 5]), (0x80, 31, [6, 6])], 2)
    assert status_of(gpu, log(rows) + [(other, IT)], []) == (5, 4)                 # pc 4 in two AIRs
    # 7: a multiplicity of 2 (row 3), and a row with a send and no receive — the smallest (air, row) is named
    twice = ref.block_log(rows, 1)
    twice[0, 3] = 2
    assert status_of(gpu, [(ref.block_log(rows, 1), IT), (twice, IT)], blocks) == (7, (1 << 32) | 3)
    col = periphery._col
    send_only = periphery._tables(0, [(col(0), [col(1), col(2)])])
    assert status_of(gpu, [(ref.block_log(rows, 1), send_only)], blocks) == (7, 0)
    # an interaction on the bus with three arguments: refused before anything runs; on another bus: the AIR is ignored
    three = periphery._tables(0, [(col(0), [col(1), col(2), col(3)])])
    s = Segment(gpu, [(ref.block_log(rows, 1), three)])
    with pytest.raises(abi.HipError):
        empirical.detect(s.seg, blocks)
    assert empirical.detect(s.seg, blocks, bus=1) == empirical.EmpiricalConstraints()
    s.close()


def test_masked_fingerprints_stay_exact(gpu):
    from powdr_amd import empirical

    counts = {0x1000: 9, 0x2000: 70}
    logs = class_edge_airs(counts, seed=6)
    blocks = [(s, 3) for s in counts]
    host = [(ref.block_log(rows, n), IT) for rows, n in zip(logs, (0, 17, 58))]
    want = ref.detect(host, blocks)
    two = [(ref.block_log([(0, 1, [3, 4]), (0, 2, [5, 6])], 2), IT)]  # data cells 0 and 1 differ in both instances
    s, s2 = Segment(gpu, host), Segment(gpu, two)
    try:
        empirical.set_fingerprint_mask(0xFF)
        try:
            got = empirical.detect(s.seg, blocks)
            assert ref.as_dict(got) == want  # exact
        except empirical.EmpiricalError as e:
            assert e.status == 6             # or refused, never wrong
        empirical.set_fingerprint_mask(1)
        try:
            got = empirical.detect(s2.seg, [(0, 1)])
            assert ref.as_dict(got) == ref.detect(two, [(0, 1)])
            assert not any((0, 3) in c and (0, 4) in c for c in got.equivalence_classes_by_block[0])
        except empirical.EmpiricalError as e:
            assert e.status == 6
        assert empirical.last_stats()["cells_verified"] > 0
    finally:
        empirical.set_fingerprint_mask(0)
        s.close()
        s2.close()
    assert ref.as_dict(run(gpu, host, blocks)) == want and empirical.last_stats()["seeds"] == 1


# ---- the chained execution: traces by powdr_original_airs_expand, bridge through the instruction AIRs' real programs ----------------------
def device_airs(gpu, table, rec, calls):
    torch, prover = gpu
    from oracle import original_chips as ooc
    from powdr_amd import original_chips as pc
    from powdr_amd import synth
    from tests import _chained_vm as vm

    itab = pc.InstructionTable(vm.BLOCK, [True] * len(vm.BLOCK), vm.START_PC)
    heights = pc.dummy_trace_heights(itab, calls)
    d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.int32).reshape(-1)).cuda()
    bufs, seg, keep, names = [None] * pc.N_KINDS, [], [d_rec], {}
    for k, h in enumerate(heights):
        if not h:
            continue
        t = torch.zeros(pc.WIDTHS[k] * h, dtype=torch.int32, device="cuda")
        bufs[k] = (t.data_ptr(), h)
        bc, sp, it = synth.reference_air_programs(ooc.KIND_NAMES[k])
        names[len(seg)] = ooc.KIND_NAMES[k]
        seg.append((prover.Prover(pc.WIDTHS[k], bc, sp, num_queries=2, interactions=it), t.data_ptr(), h.bit_length() - 1))
        keep.append(t)
    pc.expand(d_rec.data_ptr(), calls, itab, bufs)
    torch.cuda.synchronize()
    return seg, keep, names


def host_airs(ex, rec):
    from oracle import original_chips as ooc
    from powdr_amd import synth

    traces = ooc.expand_dummy_traces(ex.table, rec, ex.rbs)
    return [(t, synth.reference_air_programs(ooc.KIND_NAMES[k])[2]) for k, t in sorted(traces.items())]


def test_the_chained_execution(gpu):
    from powdr_amd import empirical
    from tests import _chained_vm as vm

    ex = vm.Execution(64, seed=3)
    blocks = [(vm.START_PC, len(vm.BLOCK))]
    seg, keep, names = device_airs(gpu, ex.table, ex.rec, 64)
    got = empirical.detect(seg, blocks, column_names={a: [f"{n}_{c}" for c in range(seg[a][0].width)] for a, n in names.items()})
    want = ref.detect(host_airs(ex, ex.rec), blocks)
    assert ref.as_dict(got) == want
    pcs = [vm.START_PC + 4 * i for i in range(len(vm.BLOCK))]
    assert got.pc_counts == {pc: 64 for pc in pcs}
    by_pc = got.debug_info["air_id_by_pc"]
    assert [names[by_pc[pc]] for pc in pcs] == ["BaseAlu", "LoadStore", "BaseAlu", "LoadStore", "LessThan", "Shift", "Multiplication", "BaseAlu", "BaseAlu", "JalLui"]
    assert len(set(by_pc.values())) == 6 and sorted(got.debug_info["column_names_by_air_id"]) == sorted(set(by_pc.values()))
    # the immediate of the two ADDIs (operand c = 1 and 4) is the same in every call: some column of each row is constant at it,
    # and the call counter x2 makes at least one column of the first ADDI move
    for i, imm in ((0, 1), (8, 4)):
        r = got.column_ranges_by_pc[pcs[i]]
        assert (imm, imm) in r and any(lo != hi for lo, hi in r)
    assert got.equivalence_classes_by_block[vm.START_PC]
    # two batches of 32 calls, combined, against the reference route treated the same way
    halves, wants = [], []
    for part in (ex.rec[:, :32], ex.rec[:, 32:]):
        seg_h, keep_h, _ = device_airs(gpu, ex.table, part, 32)
        halves.append(empirical.detect(seg_h, blocks))
        wants.append(ref.to_constraints(ref.detect(host_airs(ex, part), blocks)))
        for p, _, _ in seg_h:
            p.close()
    combined = halves[0].combine_with(halves[1])
    assert ref.as_dict(combined) == ref.as_dict(wants[0].combine_with(wants[1]))
    assert combined.pc_counts == got.pc_counts and combined.equivalence_classes_by_block == got.equivalence_classes_by_block
    for p, _, _ in seg:
        p.close()
