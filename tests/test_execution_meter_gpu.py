"""The metered cut on the GPU against the restatement of tests/_execution_meter_ref.py: every field exact — the cuts,
starts, class heights, system heights (B, M, 2 M) and every row list — with the meter's tile at 64 positions and at its default, the
statuses with their order, determinism, `system=None` against the metered call without a binding cap, and the chained execution cut
under system caps: every segment closed with the boundary, Merkle and Poseidon2 traces at the heights the cut metered, proven and chained.

The synthetic traces are tests/test_execution_segments_gpu.py's state logs (41 and 17 columns: 3 and 1 access slots) with accesses: a
slot's receive and send both count as accesses to its (as, ptr). Data words and timestamps are not read by the cut."""
import functools

import numpy as np
import pytest

from tests import _execution_meter_ref as mref
from tests import _execution_segments_ref as ref
from tests import _execution_states_ref as sref
from tests.test_execution_segments_gpu import W0, W1, Dev, piece_of, same, three_alu_block

pytestmark = pytest.mark.gpu
WIDTHS = mref.WIDTHS
SLOTS = (3, 1)
PTR_MASK = (1 << 29) - 1
FREE = (31, 31, 31)  # no system cap binds


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def of_keys(keys_at):
    """keys per position -> (as, ptr) pairs per position, hashable"""
    return tuple(tuple((1 + (int(k) >> 29), int(k) & PTR_MASK) for k in ks) for ks in keys_at)


@functools.lru_cache(maxsize=None)
def log_of(n, accesses, pattern=(0, 1, 0, 0), place_seed=1, seed=5):
    """-> (host AIRs, final pc): n positions, position i with the accesses[i] = ((as, ptr), ..); shared and left unchanged"""
    period = len(pattern)
    rng = np.random.default_rng([seed, n, 0x5e95])
    ts = (1000 + np.cumsum(rng.integers(4, 8, size=n + 1))).tolist()
    assert len(accesses) == n and all(len(a) <= SLOTS[pattern[i % period]] for i, a in enumerate(accesses))
    rows = [(4 * (i % period), ts[i], 4 * ((i + 1) % period), ts[i + 1], [(1, s, p, 0, 0, 0) for s, p in accesses[i]]) for i in range(n)]
    place = np.random.default_rng([place_seed, n, 0xd1])
    host = []
    for air, (n_access, extra) in enumerate(((3, 1), (1, 0))):
        part = [r for i, r in enumerate(rows) if pattern[i % period] == air]
        log_h = max(2, (max(len(part), 2) - 1).bit_length()) + extra
        host.append((sref.state_log(part, n_access, log_h=log_h, places=place.permutation(1 << log_h)[:len(part)]), sref.state_log_interactions(n_access)))
    assert [len(c) for c, _ in host] == [W0, W1]
    return tuple(host), 4 * (n % period)


def random_keys(n, height, pattern=(0, 1, 0, 0), seed=3):
    """up to a row's slots of accesses per position: at height 4 any key of the tree; at height 1 one of the two keys per position (two
    of them already are the whole tree); at 30 a few registers, a stream of fresh blocks and a few words of address space 2"""
    rng = np.random.default_rng([seed, n, height])
    out = []
    for i in range(n):
        m = int(rng.integers(0, SLOTS[pattern[i % len(pattern)]] + 1))
        if height == 1:
            out.append([int(rng.integers(0, 2))] * m)
        elif height < 30:
            out.append(rng.integers(0, 1 << height, size=m).tolist())
        else:
            kinds = rng.integers(0, 4, size=m).tolist()
            out.append([(4 * int(rng.integers(0, 8)), 4 * int(rng.integers(0, 8)), 0x1000 + 4 * i, (1 << 29) + 4 * int(rng.integers(0, 5)))[k] for k in kinds])
    return out


def check(gpu, host, final_pc, max_log_height, height, caps, widths=WIDTHS, calls=(), cycles=(), apc_widths=None, tiles=(64, 0), **kw):
    """the metered cut on the device at every tile size and by the restatement, compared: the result or the status -> (the
    restatement's result or None, its (status, info) or None, the meter's stats of the last run)"""
    from powdr_amd import execution_segments as es

    ref_kw = {k: v for k, v in kw.items() if k != "scratch_bytes"}
    try:
        want, err = mref.segments(host, final_pc, max_log_height, height, caps, widths, calls=calls, apc_widths=apc_widths or [0] * len(cycles), **ref_kw), None
    except mref.Status as e:
        want, err = None, (e.status, e.info)
    meter_stats = None
    with Dev(gpu, host) as d:
        for tile in tiles:
            es.set_meter_tile(tile)
            try:
                with es.cut(d.seg, max_log_height, final_pc, calls=list(calls), apcs=list(cycles), apc_widths=apc_widths, system=es.SystemMeter(height, caps, widths),
                            **kw) as got:
                    assert err is None, err
                    same(got, want, len(cycles), len(host))
                    assert got.system_heights == want["system_heights"]
                    meter_stats = es.last_meter_stats()
                    assert meter_stats["accesses"] == want["accesses"]
            except es.ExecutionSegmentsError as e:
                assert (e.status, e.info) == err
            finally:
                es.set_meter_tile(0)
            assert es.last_stats()["scratch_bytes"] == 0
    return want, err, meter_stats


# ---- sizes, tree heights, tiles ----------------------------------------------------------------------------------------------------------
CAPS_OF = {1: (0, 1, 2), 4: (2, 4, 5), 30: (3, 7, 8)}  # per tree height: caps that bind on random keys and let one position's paths in


@pytest.mark.parametrize("height", [1, 4, 30])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 1023, 1024, 1025, (1 << 12) + 1])
def test_state_logs_of_every_size(gpu, n, height):
    host, final_pc = log_of(n, of_keys(random_keys(n, height)))
    want, err, _ = check(gpu, host, final_pc, 5, height, CAPS_OF[height])
    assert err is None and want["positions"] == n
    if n == 0:
        assert want["bounds"] == [0] and want["system_heights"] == []
    if n > 1000:
        caps = CAPS_OF[height]
        assert any(b == 1 << caps[0] or m == 1 << caps[1] or p == 1 << caps[2] or m + 1 == 1 << caps[1] for b, m, p in want["system_heights"])  # a cap is reached
        assert len(want["bounds"]) > n // 64


def fresh(n):
    return of_keys([[i] for i in range(n)])


def test_a_count_exactly_at_its_cap_at_the_end_and_one_more(gpu):
    # one fresh block per position in a tree of height 4: 8 keys are 8 blocks and 5 + (1 + 2 + 1 + 3 + 1 + 2 + 1) = 16 nodes
    for caps in ((3, 31, 31), (31, 4, 31)):
        for n, segments in ((7, 1), (8, 1), (9, 2)):
            host, final_pc = log_of(n, fresh(n))
            want, err, _ = check(gpu, host, final_pc, 5, 4, caps)
            assert err is None and len(want["bounds"]) - 1 == segments, (caps, n)
        assert want["bounds"] == [0, 8, 9] and want["system_heights"] == [(8, 16, 32), (1, 5, 10)]


def test_the_poseidon2_bound_binds_first(gpu):
    host, final_pc = log_of(9, fresh(9))
    want, err, _ = check(gpu, host, final_pc, 5, 4, (31, 4, 4))  # the same cap: 2 M <= 16 binds before M <= 16
    assert err is None and want["bounds"][:2] == [0, 3] and want["system_heights"][0] == (3, 8, 16)


def test_a_system_cap_before_any_class_and_a_class_before_the_system_caps(gpu):
    n = 300
    host, final_pc = log_of(n, of_keys(random_keys(n, 30)))
    want, err, _ = check(gpu, host, final_pc, 5, 30, (3, 31, 31))
    assert err is None and all(max(h.values()) < 32 for h in want["heights"]) and all(6 <= b <= 8 for b, _, _ in want["system_heights"][:-1])  # (a position touches up to 3 blocks)
    want, err, _ = check(gpu, host, final_pc, 2, 30, (10, 20, 21))
    assert err is None and all(max(h.values()) == 4 for h in want["heights"][:-1]) and want == {**ref.segments(host, final_pc, 2), **{k: want[k] for k in ("system_heights", "accesses")}}


@pytest.mark.parametrize("height", [1, 4, 30])
def test_every_access_to_one_register(gpu, height):
    n = 257
    host, final_pc = log_of(n, of_keys([[1] * SLOTS[(0, 1, 0, 0)[i % 4]] for i in range(n)]))
    want, err, stats = check(gpu, host, final_pc, 3, height, (0, 5, 6))
    assert err is None and len(want["bounds"]) > 20 and set(want["system_heights"]) == {(1, height + 1, 2 * height + 2)}
    assert stats["accesses"] == 2 * sum(SLOTS[(0, 1, 0, 0)[i % 4]] for i in range(n))  # a slot's receive and its send


def test_every_access_to_a_fresh_block_and_a_table_that_grows(gpu):
    n = (1 << 12) + 1
    host, final_pc = log_of(n, of_keys([[i << 16] for i in range(n)]))  # blocks 2^16 apart: 16 nodes of its own under every block
    want, err, stats = check(gpu, host, final_pc, 20, 30, FREE, tiles=(64, 0, 1 << 20))  # one segment: the table holds every node
    assert err is None and want["bounds"] == [0, n] and want["system_heights"][0][0] == n
    assert want["system_heights"][0][1] == mref.merkle_closed_form([i << 16 for i in range(n)], 30) > 16 * n
    assert stats["tables"] > 1 and stats["table_peak_slots"] > 1 << 16 and stats["nodes_past_the_cuts"] == 0  # the first table of 2^16 slots overflowed
    want, err, stats = check(gpu, host, final_pc, 20, 30, (6, 31, 31))
    assert err is None and len(want["bounds"]) - 1 == -(-n // 64) and stats["tiles"] >= len(want["bounds"]) - 1 and stats["synchronisations"] > stats["tiles"]


def test_keys_that_differ_in_the_top_bit_and_both_address_spaces(gpu):
    for height in (1, 4, 30):
        top = 1 << (height - 1)
        keys = [[0], [top], [0, top], [top], [1 if height > 1 else 0], [top + (1 if height > 1 else 0)]] * 3
        host, final_pc = log_of(len(keys), of_keys(keys), pattern=(0,))
        want, err, _ = check(gpu, host, final_pc, 5, height, FREE)
        assert err is None and want["system_heights"][0][1] == mref.merkle_closed_form([k for ks in keys for k in ks], height)
        want, err, _ = check(gpu, host, final_pc, 5, height, (1, 31, 31))
        assert err is None and (len(want["bounds"]) > 2 or height == 1)  # (a tree of height 1 has two blocks)
    acc = ((1, 8), (2, 8)), ((2, 8),), ((1, 8),), ((2, 12), (1, 12))  # the same pointers in both address spaces
    host, final_pc = log_of(4, acc, pattern=(0,))
    want, err, _ = check(gpu, host, final_pc, 5, 30, FREE)
    assert err is None and want["system_heights"] == [(4, 31 + 3 + 30 + 3, 134)]  # (keys 8, 12, 2^29 + 8, 2^29 + 12)


# ---- calls ------------------------------------------------------------------------------------------------------------------------------
def test_a_new_block_inside_a_call_moves_the_cut_to_the_calls_start(gpu):
    from powdr_amd import execution_segments as es

    keys = [[0], [1], [0], [1], [], [], [2], [], [3], [2], [3], [2]]
    host, final_pc = log_of(12, of_keys(keys), pattern=(0,))
    want, err, _ = check(gpu, host, final_pc, 5, 4, (1, 31, 31), calls=[(0, 4, 8)], cycles=[4])
    assert err is None and want["bounds"] == [0, 4, 12] and want["snapped"] == 1 and es.last_stats()["snapped_cuts"] == 1  # (same() compares the count with the walk's)
    assert want["system_heights"][0][0] == 2 and want["heights"][1] == {("apc", 0): 1, 0: 4}
    # the call starts at b_s: the moved cut lands on b_s
    keys = [[0], [1], [2], [3], [0], [0]]
    host, final_pc = log_of(6, of_keys(keys), pattern=(0,))
    assert check(gpu, host, final_pc, 5, 4, (1, 31, 31), calls=[(0, 0, 4)], cycles=[4])[1] == (13, 0)
    keys = [[0], [0], [0], [1], [2], [0]]
    host, final_pc = log_of(6, of_keys(keys), pattern=(0,))
    assert check(gpu, host, final_pc, 5, 4, (0, 31, 31), calls=[(0, 2, 6)], cycles=[4])[1] == (13, 2)  # b_1 = 2, then the call's second block
    # random calls and caps: the counts of the moved cuts equal the walk's (same()) and some cut moves
    rng = np.random.default_rng(78)
    host, final_pc = log_of(300, of_keys(random_keys(300, 30)))
    moved = 0
    for _ in range(4):
        calls, at = [], 0
        while True:
            a = int(rng.integers(0, 2))
            at += int(rng.integers(0, 9))
            if at + (5, 9)[a] > 300:
                break
            calls.append((a, at, at + (5, 9)[a]))
            at += (5, 9)[a]
        want, err, _ = check(gpu, host, final_pc, 3, 30, (4, 31, 31), calls=calls, cycles=[5, 9], tiles=(64,))
        assert err is None and all(ref.allowed(300, calls)[b] for b in want["bounds"])
        moved += want["snapped"]
    assert moved > 0


def test_one_position_whose_paths_exceed_the_merkle_cap(gpu):
    keys = [[8], [8], [8, 12]]
    host, final_pc = log_of(3, of_keys(keys), pattern=(0,))
    assert check(gpu, host, final_pc, 5, 30, (31, 4, 31))[1] == (13, 0)  # 31 nodes against 16, without max_cells
    assert check(gpu, host, final_pc, 5, 30, (31, 5, 31))[1] == (13, 2)  # [0, 2) holds 31 nodes; position 2 alone 33
    assert check(gpu, host, final_pc, 5, 30, (31, 31, 5))[1] == (13, 0)  # 62 against 32: the bound


# ---- max_cells --------------------------------------------------------------------------------------------------------------------------
def test_the_cell_budget_with_the_system_terms(gpu):
    host, final_pc = log_of(9, fresh(9), pattern=(0,))
    run = lambda widths, cells, height=4: check(gpu, host, final_pc, 5, height, FREE, widths, max_cells=cells)
    # widths (10, 0, 0): q positions cost 41 padded(q) + 10 padded_sys(q) = 61, 102, 204, 204, 408: exactly at the jump and one below
    assert run((10, 0, 0), 204)[0]["bounds"][:2] == [0, 4] and run((10, 0, 0), 203)[0]["bounds"][:2] == [0, 2]
    assert run((10, 0, 0), 61)[0]["bounds"][:2] == [0, 1] and run((10, 0, 0), 60)[1] == (13, 0)  # padded_sys(1) = 2
    # the Poseidon2 term alone binds: 2 M = 10, 12, 16, 18 is padded to 16, 16, 16, 32; the classes alone cost 164 at four positions
    assert run((0, 0, 1), 195)[0]["bounds"][:2] == [0, 3] and run((0, 0, 1), 196)[0]["bounds"][:2] == [0, 4]
    assert run((0, 0, 0), 195)[0]["bounds"][:2] == [0, 4]  # width 0 leaves the term out
    assert run((0, 5, 0), 164 + 5 * 16)[0]["bounds"][:2] == [0, 4] and run((0, 5, 0), 164 + 5 * 16 - 1)[0]["bounds"][:2] == [0, 3]  # M = 9 is padded to 16
    # the real widths, a budget of 2^64 - 1 and sums that saturate; min_log_height pads the system terms too
    assert run(WIDTHS, (1 << 64) - 1)[0]["bounds"] == [0, 9]
    assert run(((1 << 32) - 1,) * 3, (1 << 40), 30)[0] is not None
    want, err, _ = check(gpu, host, final_pc, 5, 4, FREE, (1, 0, 0), max_cells=41 * 8 + 8, min_log_height=3)
    assert err is None and want["bounds"][:2] == [0, 8]
    # with calls and random budgets against the walk
    n = 300
    host2, final_pc2 = log_of(n, of_keys(random_keys(n, 30)))
    calls = [(0, 9 * j, 9 * j + 5) for j in range(30)]
    probes = 0
    for cells in (90000, 150000, 300000):  # (one position: 307 * 64 cells of the Poseidon2 bound and more)
        want, err, _ = check(gpu, host2, final_pc2, 4, 30, (4, 8, 9), calls=calls, cycles=[5], apc_widths=[9], max_cells=cells, tiles=(64,))
        assert err is None
        probes += len(want["bounds"])
    assert probes > 10


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_status_15_by_each_cause_with_the_smallest_witness(gpu):
    from powdr_amd import stage

    good = ((1, 8),), ((2, 4),), ((1, 12),), ((1, 8),)
    for height, bad in ((30, (3, 8)), (30, (0, 8)), (30, (1, 1 << 29)), (30, (2, (1 << 29) + 4)), (4, (1, 16)), (4, (2, 0)), (1, (1, 2))):
        acc = list(good) if height == 30 else [((1, 1),)] * 4
        acc[2] = (bad,)
        host, final_pc = log_of(4, tuple(acc), pattern=(0,))
        _, err, _ = check(gpu, host, final_pc, 5, height, FREE)
        assert err is not None and err[0] == 15, (height, bad)
        air, inter, row = stage.unpack_witness(err[1])
        cols = host[0][0]
        assert air == 0 and inter == 2 and (int(cols[6, row]), int(cols[7, row])) == bad  # the slot's receive, before its send
    # two of them: the smaller (air, interaction, row) is named — an AIR 0 access against AIR 1's
    acc = [((1, 8),), ((3, 8),), ((1, 8), (1, 12), (5, 0)), ((1, 8),)]
    host, final_pc = log_of(4, tuple(acc))
    _, err, _ = check(gpu, host, final_pc, 5, 30, FREE)
    assert err[0] == 15 and stage.unpack_witness(err[1])[:2] == (0, 6)  # AIR 0, its third slot's receive (interactions 2 + 2 * 2)


def test_status_2_and_a_run_inside_the_bytes_it_names(gpu):
    from powdr_amd import execution_segments as es

    n = 1025
    host, final_pc = log_of(n, of_keys(random_keys(n, 30)))
    calls = [(0, 9 * j, 9 * j + 5) for j in range(100)]
    args = dict(calls=calls, apcs=[5], apc_widths=[9], max_cells=150000, system=es.SystemMeter(30, (4, 8, 9)))
    with Dev(gpu, host) as d:
        with pytest.raises(es.ExecutionSegmentsError) as e:
            es.cut(d.seg, 3, final_pc, scratch_bytes=1 << 16, **args)
        assert e.value.status == 2 and e.value.info > 1 << 16 and es.last_stats()["scratch_bytes"] == 0
        need = e.value.info
        with es.cut(d.seg, 3, final_pc, scratch_bytes=need, **args) as inside, es.cut(d.seg, 3, final_pc, **args) as free:
            assert 0 < es.last_stats()["peak_bytes"] <= need
            assert (inside.bounds, inside.system_heights, inside.heights) == (free.bounds, free.system_heights, free.heights) and len(free.bounds) > 10
        with pytest.raises(es.ExecutionSegmentsError) as e:
            es.cut(d.seg, 3, final_pc, scratch_bytes=need - 1, **args)
        assert (e.value.status, e.value.info) == (2, need)
    assert es.last_stats()["scratch_bytes"] == 0


def test_the_status_order_2_7_4_11_15_13_14(gpu):
    from powdr_amd import execution_segments as es

    it = sref.state_log_interactions(1)
    row = lambda i, ts, acc: (4 * i, ts, 4 * i + 4, ts + 5, [(1, *acc, 0, 0, 0)])
    rows = [row(0, 10, (1, 8)), row(1, 20, (3, 8)), row(2, 30, (1, 12)), row(3, 40, (1, 16))]  # position 1: no key
    late = [(0, 0, 2), (0, 3, 5)]
    caps = (0, 31, 31)

    def status(rows, tamper=None, **kw):
        cols = sref.state_log(rows, 1)
        if tamper:
            tamper(cols)
        host = [(cols, it)]
        return check(gpu, host, 16, 5, 30, kw.pop("caps", caps), **kw)[1]

    assert status(rows, calls=late, cycles=[2]) == (11, 1)  # 11 before 15
    assert status(rows) is not None and status(rows)[0] == 15  # 15 before 13
    assert status(rows, max_segments=1)[0] == 15  # and before 14
    assert status(rows + [row(4, 40, (1, 8))], calls=late, cycles=[2]) == (4, 40)  # a duplicate time key: before 11 and 15

    def twice(cols):
        cols[0, 1] = 2

    assert status(rows + [row(4, 40, (1, 8))], twice, calls=late, cycles=[2]) == (7, 1)  # a multiplicity of 2: before the duplicate
    ok = [row(0, 10, (1, 8)), row(1, 20, (1, 8)), row(2, 30, (1, 12)), row(3, 40, (1, 16))]
    assert status(ok) is None and status(ok, max_segments=2) == (14, 3) and status(ok, max_segments=3) is None  # [0, 2) [2, 3) [3, 4)
    both = [row(0, 10, (1, 8)), row(1, 20, (1, 12)), row(2, 30, (1, 12)), row(3, 40, (1, 16))]
    assert status(both, caps=(31, 4, 31)) == (13, 0) and status(both, caps=(31, 4, 31), max_segments=1) == (13, 0)
    with Dev(gpu, [(sref.state_log(rows + [row(4, 40, (1, 8))], 1), it)]) as d:
        with pytest.raises(es.ExecutionSegmentsError) as e:  # 2 before everything
            es.cut(d.seg, 5, 16, calls=late, apcs=[2], scratch_bytes=1 << 12, system=es.SystemMeter(30, caps))
        assert e.value.status == 2
        with pytest.raises(es.stage.Malformed, match="pw_execution_segments_from_traces_metered: malformed arguments"):
            es.cut(d.seg, 5, 16, system=es.SystemMeter(30, caps, memory_bus=0))  # the bridge's interactions have two arguments, not 7
    assert es.last_stats()["scratch_bytes"] == 0


# ---- determinism, order independence, and the unmetered call ---------------------------------------------------------------------------
def test_two_runs_are_identical_and_the_row_order_does_not_matter(gpu):
    from powdr_amd import execution_segments as es

    n = 1025
    acc = of_keys(random_keys(n, 30))
    calls = [(j % 3, 11 * j, 11 * j + 4) for j in range(90)]
    seen = []
    for place_seed in (1, 1, 2):
        host, final_pc = log_of(n, acc, place_seed=place_seed)
        with Dev(gpu, host) as d, es.cut(d.seg, 3, final_pc, calls=calls, apcs=[4, 4, 4], apc_widths=[5, 50, 500], max_cells=150000, system=es.SystemMeter(30, (4, 8, 9))) as got:
            lists = {k: v.tobytes() for k, v in got.read_lists().items()}
            seen.append((got.bounds, got.starts, got.heights, got.system_heights, got.first_call, got.final_pc, lists))
    assert seen[0] == seen[1] and len(seen[0][0]) > 20
    assert seen[0][:6] == seen[2][:6] and seen[0][6] != seen[2][6] and sorted(seen[0][6]) == sorted(seen[2][6])  # other rows, the same cut


def test_system_none_is_the_unmetered_call(gpu):
    from powdr_amd import execution_segments as es

    n = 1025
    host, final_pc = log_of(n, of_keys(random_keys(n, 30)))
    calls = [(0, 9 * j, 9 * j + 5) for j in range(100)]
    args = dict(calls=calls, apcs=[5], apc_widths=[9], max_cells=4000)
    want = ref.segments(host, final_pc, 3, calls, [9], max_cells=4000)
    with Dev(gpu, host) as d:
        with es.cut(d.seg, 3, final_pc, system=None, **args) as plain:
            same(plain, want, 1)
            assert plain.system_heights == [(0, 0, 0)] * plain.n_segments and es.last_meter_stats() == dict.fromkeys(es.METER_STATS, 0)
            plain_lists = {k: v.tobytes() for k, v in plain.read_lists().items()}
            # the metered entry point with no system limit in the way gives the same cut, and says what the segments touch
            with es.cut(d.seg, 3, final_pc, system=es.SystemMeter(30, 31, (0, 0, 0)), **args) as metered:
                same(metered, want, 1)
                assert {k: v.tobytes() for k, v in metered.read_lists().items()} == plain_lists
                assert metered.system_heights == mref.segments(host, final_pc, 3, 30, 31, (0, 0, 0), calls=calls, apc_widths=[9], max_cells=4000)["system_heights"]
                assert all(b > 0 for b, _, _ in metered.system_heights)
    assert es.last_stats()["scratch_bytes"] == 0


# ---- the chained execution ------------------------------------------------------------------------------------------------------------------
def test_the_chained_execution_cut_under_system_caps_closed_proven_and_chained(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import execution_segments as es
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa
    from tests import _chained_vm as vm
    from tests import test_system_airs_gpu as tsa
    from tests.test_memory_merkle_gpu import H, closed_with, constants, statement
    from tests.test_memory_tree_gpu import leaf_of

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex = vm.Execution(48, seed=5, block=three_alu_block())
    airs = ex.instruction_airs()
    host = [(t, programs[2]) for _, t, programs in airs]
    leaves = dict(leaf_of(loc, word) for loc, (word, _) in ex.initial.items())
    keys0 = np.array(sorted(leaves), np.uint64)
    pay0 = np.array([leaves[int(x)] for x in keys0], np.uint32)
    class_cap, caps = 6, (5, 7, 8)  # 32 blocks, 128 nodes, a bound of 256 hashes; the class cap alone gives segments of 164 nodes
    valid = sa.BOUNDARY_COLUMNS.index("is_valid")

    def system_rows(c):
        b, m = c.by_name("boundary"), c.by_name("memory_merkle")
        count = lambda a, col: int((a["trace"].view(a["width"], -1)[col] != 0).sum())
        return (count(b, valid), b["log_h"]), (count(m, 0), m["log_h"]), c.by_name("poseidon2")["log_h"]

    with Dev(gpu, host) as d:
        # the gap: cut by the classes alone, a segment's Merkle trace is taller than the system cap
        with es.cut(d.seg, class_cap, ex.end[0], system=None) as plain:
            assert plain.bounds == ref.segments(host, ex.end[0], class_cap)["bounds"]
            tree = mt.MemoryTree(H)
            assert tree.load(keys0, pay0) == (0, 0)
            c = closed_with(gpu, piece_of(ex, airs, plain.segment(0)), public_connector=True, poseidon2=True, memory_tree=tree)
            (_, _), (nodes, merkle_lh), _ = system_rows(c)
            assert nodes > 1 << caps[1] and merkle_lh > caps[1]
            c.close()
            tree.close()
        want = mref.segments(host, ex.end[0], class_cap, H, caps)
        with es.cut(d.seg, class_cap, ex.end[0], system=es.SystemMeter(H, caps)) as got:
            same(got, want, 0, len(host))
            S = got.n_segments
            assert got.system_heights == want["system_heights"] and S > plain.n_segments and got.positions == 48 * 9
            assert max(m for _, m, _ in got.system_heights) > (1 << caps[1]) - 8 and all(max(h.values()) < 1 << class_cap for h in got.heights)  # the Merkle cap binds
            tree = mt.MemoryTree(H)
            assert tree.load(keys0, pay0) == (0, 0)
            closed, segments = [], []
            for s in range(S):
                B, M, P2 = got.system_heights[s]
                c = closed_with(gpu, piece_of(ex, airs, got.segment(s)), public_connector=True, poseidon2=True, memory_tree=tree)
                closed.append(c)
                (locations, boundary_lh), (nodes, merkle_lh), poseidon2_lh = system_rows(c)
                assert locations == B and 1 << boundary_lh == es.padded_sys(B), s
                assert nodes == M and 1 << merkle_lh == es.padded_sys(M), s
                assert 1 << poseidon2_lh <= es.padded_sys(P2), s
                assert boundary_lh <= caps[0] and merkle_lh <= caps[1] and poseidon2_lh <= caps[2]
                summaries, tuples = prover.check_segment_buses(c.seg)
                assert [(x["bus"], x["status"]) for x in summaries] == [(b, 0) for b in (0, 1, 2, 3, 5, 6, 7, 8, 9)] and tuples == []
                for a in c.airs:
                    assert a["prover"].check_constraints(a["trace"].data_ptr(), a["log_h"]) == (0, None, None), (s, a["name"])
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
    whole = mt.MemoryTree(H)
    assert whole.load(keys0, pay0) == (0, 0)
    closed_with(gpu, ex, public_connector=True, poseidon2=True, memory_tree=whole).close()
    assert (whole.root() == last_root).all()
    whole.close()
