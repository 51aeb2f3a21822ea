"""Direct mode of apply_calls on the GPU: the named columns of the APC traces, written straight from the chips' traces by
pw_apc_sources_tracegen, word for word against the restatement of tests/_apc_direct_ref.py AND against the two-step path (a flags-0
handle, then powdr_apc_tracegen_host_tables on its source matrices) of the same inputs. Outputs are pre-filled with 0xA5A5A5A5: a column
no cell names must still hold it.

The traces are state logs as in tests/test_apc_sources_gpu.py, with a strictly periodic program so that the number of calls is chosen
exactly: position i runs instruction i mod period, the AIR of an instruction is PATTERN[...][instruction], the APC is the first
`length` instructions of the period and call j covers the positions j * period .. j * period + length - 1."""
import functools

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _apc_direct_ref as dref
from tests import _apc_sources_ref as ref
from tests import _execution_states_ref as sref
from tests.test_apc_sources_gpu import gpu, tracegen  # noqa: F401  (the fixture; the two-step path's second step)

pytestmark = pytest.mark.gpu
FILL_I32 = int(np.uint32(dref.FILL).view(np.int32))
# name -> (the AIR of every instruction of the period, the APC's length). AIR 1 holds ONE instruction per period wherever the 16-byte
# path is wanted: in time order its rows of consecutive calls are consecutive rows.
PATTERN = {1: ([1, 0, 0], 2),              # rbs 1 in both AIRs
           2: ([0, 1, 0, 0], 3),           # AIR 0: rbs 2, occ 0 and 1
           3: ([0, 1, 0, 0, 0], 4),        # AIR 0: rbs 3, occ 0, 1, 2
           "alt": ([0, 1, 0, 1, 0, 0], 5)}  # alternating: AIR 0 rbs 3, AIR 1 rbs 2


@functools.lru_cache(maxsize=None)
def periodic_log(n_calls, pattern, random_rows=True, tail=3, n_access=3, seed=5):
    """-> (host AIRs [(cols canonical, interactions)] of two state logs of different heights, the same with Montgomery words, the calls)"""
    airs_of, length = PATTERN[pattern]
    period = len(airs_of)
    n = n_calls * period + tail
    ex = sref.Execution(n, seed=seed, n_access=n_access)
    rows = [(4 * (i % period), ts, 4 * ((i + 1) % period), nts, acc) for i, (_, ts, _, nts, acc) in enumerate(ex.rows)]
    it = sref.state_log_interactions(n_access)
    place = np.random.default_rng([seed, n, 0xd1])
    host = []
    for air, extra in ((0, 1), (1, 0)):
        part = [r for r in rows if airs_of[r[0] // 4] == air]
        log_h = max(2, (max(len(part), 2) - 1).bit_length()) + extra
        places = place.permutation(1 << log_h)[:len(part)] if random_rows else np.arange(len(part))
        host.append((sref.state_log(part, n_access, log_h=log_h, places=places), it))
    monty = [(om.to_monty(np.ascontiguousarray(cols)).reshape(cols.shape), it) for cols, it in host]
    return host, monty, [(0, j * period, j * period + length) for j in range(n_calls)]


def outputs(torch, handle, specs, offset=0):
    """one apc_traces call for specs [(apc, cells, out_height, out_width)] -> the raw words [out_width, out_height] per job; offset: the
    matrices begin that many words into their (16-byte aligned) buffers"""
    bufs = [torch.full((w * h + offset,), FILL_I32, dtype=torch.int32, device="cuda") for _, _, h, w in specs]
    torch.cuda.synchronize()
    handle.apc_traces([(a, cells, b.data_ptr() + 4 * offset, h, w) for (a, cells, h, w), b in zip(specs, bufs)])
    got = [b.cpu().numpy().view(np.uint32) for b in bufs]
    assert all((g[:offset] == dref.FILL).all() for g in got)
    return [g[offset:].reshape(w, h) for g, (_, _, h, w) in zip(got, specs)]


def two_step(torch, plain, spec):
    """the parent interface on the same cells: the flags-0 handle's matrices through powdr_apc_tracegen_host_tables -> raw [w, h]"""
    apc, cells, h, w = spec
    return tracegen(torch, plain.original_airs(apc), len(plain.source_airs(apc)), plain.substs(apc, cells), h, w, plain.layout[apc].n_calls)


class Applied:
    """a segment on the device with a direct and a flags-0 handle of the same calls, and the restatement"""

    def __init__(self, gpu, host, monty, cycles, calls, **kw):
        from powdr_amd import apc_sources as aps
        from tests.test_bus_check_gpu import Segment

        self.torch, self.monty = gpu[0], monty
        self.s = Segment(gpu, host)
        self.direct = self.plain = None
        try:
            self.direct = aps.apply_calls(self.s.seg, calls, cycles, direct=True, **kw)
            self.plain = aps.apply_calls(self.s.seg, calls, cycles, **kw)
            self.layout, self.lists = dref.lists(host, cycles, calls)
        except BaseException:
            self.close()
            raise
        self.widths = [len(cols) for cols, _ in host]

    def check(self, specs, offset=0):
        """one call for all specs; every job against the restatement (all columns, the fill included) and the two-step path (named columns)"""
        got = outputs(self.torch, self.direct, specs, offset)
        for k, (spec, g) in enumerate(zip(specs, got)):
            apc, cells, h, w = spec
            want = dref.traces(self.monty, self.layout, self.lists, apc, cells, h, w)
            assert (g == want).all(), (k, apc, h, w, np.argwhere(g != want)[:4].tolist())
            named = sorted({c for _, _, c in cells})
            assert (g[[c for c in range(w) if c not in set(named)]] == dref.FILL).all()
            if self.layout[apc][0] and cells:
                assert (two_step(self.torch, self.plain, spec)[named] == g[named]).all(), (k, apc, h, w)
        return got

    def close(self):
        for h in (self.direct, self.plain):
            if h is not None:
                h.close()
        self.s.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def applied(gpu, n_calls, pattern, random_rows=True, **kw):
    host, monty, calls = periodic_log(n_calls, pattern, random_rows)
    return Applied(gpu, host, monty, [PATTERN[pattern][1], 1], calls, **kw)  # (APC 1 has no call)


def pow2(n):
    return ref.pow2_at_least(n)


@pytest.mark.parametrize("pattern", [1, 2, 3])
@pytest.mark.parametrize("n_calls", [0, 1, 3, 4, 5, 1023, 1024, 1025])
def test_every_cell_at_the_next_power_of_two_and_four_times_it(gpu, n_calls, pattern):
    from powdr_amd import apc_sources as aps

    with applied(gpu, n_calls, pattern) as ap:
        length = PATTERN[pattern][1]
        cells = dref.all_cells(ap.layout, 0, ap.widths) if n_calls else [(k, c, k * 41 + c) for k in range(length) for c in range(41)]
        assert len(cells) == 41 * length
        if n_calls:  # every occ of every rbs
            by_air = {}
            for air, occ in ap.layout[0][1]:
                by_air.setdefault(air, []).append(occ)
            assert sorted(len(v) for v in by_air.values()) == [1, pattern] and all(v == list(range(len(v))) for v in by_air.values())
        h = pow2(n_calls)
        got = ap.check([(0, cells, h, len(cells)), (0, cells, 4 * h, len(cells) + 2)])
        stats = aps.tracegen_last_stats()
        assert stats["jobs"] == 2 and stats["scratch_bytes"] == 0 and stats["bytes_written"] == 4 * len(cells) * 5 * h
        assert stats["work_items"] == 2 * length * 3  # 41 cells of an instruction: groups of 16, 16 and 9
        assert got[1][:, :n_calls].any() == bool(n_calls) and not got[1][:len(cells), n_calls:].any()
    assert aps.last_stats()["scratch_bytes"] == 0 and aps.tracegen_last_stats()["scratch_bytes"] == 0


@pytest.mark.parametrize("n_calls, h", [(0, 1), (1, 1), (1, 2), (2, 2), (0, 2)])
def test_heights_one_and_two_go_word_by_word(gpu, n_calls, h):
    from powdr_amd import apc_sources as aps

    with applied(gpu, n_calls, 3) as ap:
        cells = dref.all_cells(ap.layout, 0, ap.widths) if n_calls else [(k, c, 3 * c + k) for k in range(3) for c in range(0, 41, 5)]
        ap.check([(0, cells, h, 200)])
        stats = aps.tracegen_last_stats()
        assert stats["tiles_16_byte_loads"] == 0 and stats["tiles_4_byte_loads"] == stats["work_items"] > 0


@pytest.mark.parametrize("n_calls", [5, 1025])
def test_an_output_four_bytes_off_the_grid(gpu, n_calls):
    from powdr_amd import apc_sources as aps

    with applied(gpu, n_calls, 2) as ap:
        cells = dref.all_cells(ap.layout, 0, ap.widths)
        ap.check([(0, cells, pow2(n_calls), len(cells)), (0, cells[::3], 4 * pow2(n_calls), len(cells))], offset=1)
        stats = aps.tracegen_last_stats()
        assert stats["tiles_16_byte_loads"] == 0 and stats["tiles_4_byte_loads"] > 0


@pytest.mark.parametrize("random_rows", [True, False])
def test_an_apc_alternating_between_two_airs_of_different_heights(gpu, random_rows):
    with applied(gpu, 1025, "alt", random_rows) as ap:
        assert ap.layout[0] == (1025, [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]) and ap.layout[1] == (0, [])
        assert len(ap.monty[0][0][0]) != len(ap.monty[1][0][0])
        cells = dref.all_cells(ap.layout, 0, ap.widths)
        ap.check([(0, cells, 2048, len(cells)), (1, [(0, 3, 1)], 4, 2)])  # and an APC without calls beside it: zeros


def test_cell_selections(gpu):
    """one per instruction; none for some instruction; 17 and 33 cells of one instruction (a group boundary inside it); one source cell
    into two APC columns; the cells in shuffled order — six jobs of one call"""
    from powdr_amd import apc_sources as aps

    rng = np.random.default_rng(0xce11)
    with applied(gpu, 1025, 3) as ap:
        every = dref.all_cells(ap.layout, 0, ap.widths)
        one_each = [(k, int(rng.integers(0, 41)), k) for k in range(4)]
        none_for_1_and_3 = [(k, c, c + 41 * (k // 2)) for k in (0, 2) for c in range(41)]
        seventeen = [(2, c, 16 - i) for i, c in enumerate(rng.permutation(41)[:17].tolist())]
        thirty_three = [(1, c, 2 * i) for i, c in enumerate(rng.permutation(41)[:33].tolist())] + [(3, 40, 1)]
        twice = [(0, 7, 0), (0, 7, 5), (3, 40, 2), (3, 40, 3), (3, 40, 9), (1, 0, 4)]
        shuffled = [every[i] for i in rng.permutation(len(every)).tolist()]
        specs = [(0, one_each, 2048, 4), (0, none_for_1_and_3, 2048, 90), (0, seventeen, 2048, 17), (0, thirty_three, 8192, 70), (0, twice, 2048, 10),
                 (0, shuffled, 2048, len(every))]
        got = ap.check(specs)
        stats = aps.tracegen_last_stats()
        assert stats["jobs"] == 6 and stats["work_items"] == 4 + 2 * 3 + 2 + (3 + 1) + 3 + 4 * 3
        assert stats["bytes_written"] == 4 * sum(len(cells) * h for _, cells, h, _ in specs)
        assert (got[4][0] == got[4][5]).all() and (got[4][2] == got[4][3]).all() and (got[4][3] == got[4][9]).all() and got[4][0].any()
        assert (got[5] == ap.check([(0, every, 2048, len(every))])[0]).all()  # the order of the cells does not matter


def test_time_order_loads_16_bytes_and_random_rows_load_4(gpu):
    """cells of the instruction that lies in AIR 1 (one row per period): in time order call r reads row r, four calls are one aligned
    16-byte load and no tile needs another; at random rows every tile loads words"""
    from powdr_amd import apc_sources as aps

    seen = []
    for random_rows in (False, True):
        with applied(gpu, 1024, 3, random_rows) as ap:
            assert ap.layout[0][1][1] == (1, 0)
            cells = [(1, c, c) for c in range(41)]
            seen.append(ap.check([(0, cells, 1024, 41), (0, cells, 4096, 41)]))
            stats = aps.tracegen_last_stats()
            assert stats["work_items"] == 6 and stats["tiles_16_byte_loads"] + stats["tiles_4_byte_loads"] == 3 + 3 * 4
            if random_rows:
                assert stats["tiles_4_byte_loads"] == 6 and stats["tiles_16_byte_loads"] == 9  # (zero tiles load nothing)
            else:
                assert stats["tiles_4_byte_loads"] == 0 and stats["tiles_16_byte_loads"] == 15
            every = dref.all_cells(ap.layout, 0, ap.widths)
            seen[-1] += ap.check([(0, every, 1024, len(every))])
    # the same input under two row orders gives the same traces
    assert all((a == b).all() for a, b in zip(*seen)) and seen[0][2].any()


def three_apc_log(n=600, seed=11):
    """period 6 with three APCs: instructions 0-1, 2-4 and 5 — every position covered but the tail"""
    airs_of, period = [0, 1, 1, 0, 1, 0], 6
    ex = sref.Execution(n, seed=seed)
    rows = [(4 * (i % period), ts, 4 * ((i + 1) % period), nts, acc) for i, (_, ts, _, nts, acc) in enumerate(ex.rows)]
    it = sref.state_log_interactions(ex.n_access)
    place = np.random.default_rng([seed, n])
    host = []
    for air in (0, 1):
        part = [r for r in rows if airs_of[r[0] // 4] == air]
        host.append((sref.state_log(part, ex.n_access, log_h=10, places=place.permutation(1 << 10)[:len(part)]), it))
    calls = [(a, j * period + b, j * period + e) for a, (b, e) in enumerate([(0, 2), (2, 5), (5, 6)]) for j in range(n // period - (a == 2))]
    calls.sort(key=lambda c: c[1])
    return host, [(om.to_monty(np.ascontiguousarray(cols)).reshape(cols.shape), it) for cols, it in host], [2, 3, 1], calls


def test_three_apcs_are_three_jobs_of_one_launch_and_forty_one_tile_jobs(gpu):
    from powdr_amd import apc_sources as aps

    host, monty, cycles, calls = three_apc_log()
    with Applied(gpu, host, monty, cycles, calls) as ap:
        assert [l[0] for l in ap.layout] == [100, 100, 99] and ap.layout[1][1] == [(1, 0), (0, 0), (1, 1)]
        specs = [(a, dref.all_cells(ap.layout, a, ap.widths), 128 << a, 41 * cycles[a] + a) for a in range(3)]
        ap.check(specs)
        stats = aps.tracegen_last_stats()
        assert stats["jobs"] == 3 and stats["work_items"] == 3 * (2 + 3 + 1) and stats["tiles_16_byte_loads"] + stats["tiles_4_byte_loads"] == stats["work_items"]
        rng = np.random.default_rng(40)
        forty = []
        for k in range(40):
            a = k % 3
            instr = int(rng.integers(0, cycles[a]))
            cols = rng.permutation(41)[:int(rng.integers(1, 17))].tolist()
            forty.append((a, [(instr, c, i) for i, c in enumerate(cols)], 128 << (k % 4), len(cols) + k % 2))
        ap.check(forty)
        stats = aps.tracegen_last_stats()
        assert stats["jobs"] == 40 and stats["work_items"] == 40 and stats["tiles_16_byte_loads"] + stats["tiles_4_byte_loads"] == 40
        # layout and residuals are the flags-0 handle's; a direct handle has no source matrix
        d, p = ap.direct, ap.plain
        assert d.direct and not p.direct and d.layout == p.layout and (d.positions, d.covered, d.residual_bytes) == (p.positions, p.covered, p.residual_bytes)
        assert d.source_bytes == 0 and p.source_bytes > 0 and p.index_bytes == 0 and d.index_bytes >= 4 * d.covered > 0
        for a in range(3):
            for air in range(2):
                sd, sp = d.source(a, air), p.source(a, air)
                assert sd.height == 0 and sd.ptr is None and (sd.width, sd.rbs) == (sp.width, sp.rbs) and d.read_source(a, air).size == 0
                assert aps.lib.pw_apc_sources_read_source(d._h, a, air, np.zeros(4, np.uint32).ctypes.data) == 0
        for air in range(2):
            assert tuple(d.residual(air))[1:] == tuple(p.residual(air))[1:] and (d.read_residual(air) == p.read_residual(air)).all()
        with pytest.raises(ValueError, match="apc_traces"):
            d.original_airs(0)
        with pytest.raises(ValueError, match="apc_traces"):
            d.substs(0, [(0, 0, 0)])
    assert aps.last_stats()["scratch_bytes"] == 0 and aps.tracegen_last_stats()["scratch_bytes"] == 0


def test_an_output_whose_last_column_lies_past_byte_2_to_the_32(gpu):
    torch, _ = gpu
    h, w = 1 << 24, 65
    with applied(gpu, 1025, 3) as ap:
        cells = [(0, 3, 0), (1, 2, 64), (3, 40, 1), (2, 0, 33)]
        out = torch.full((w * h,), FILL_I32, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ap.direct.apc_traces([(0, cells, out.data_ptr(), h, w)])
        m = out.view(w, h)
        want = dref.traces(ap.monty, ap.layout, ap.lists, 0, cells, 2048, w)
        named = sorted(c for _, _, c in cells)
        assert (m[:, :2048].cpu().numpy().view(np.uint32) == want).all() and want[64, :1025].any()
        assert not bool(m[named, 2048:].any()) and bool((m[[c for c in range(w) if c not in named]] == FILL_I32).all())
        theirs = two_step(torch, ap.plain, (0, cells, 2048, w))
        assert (theirs[named] == want[named]).all()
        del out, m


def test_a_source_air_of_2_to_the_24_rows_whose_last_column_is_read(gpu):
    """65 columns of 2^24 rows: column 64 begins at byte 2^32. The few active rows lie at random rows of the big AIR; what is expected
    comes from the same rows in a small AIR, because a trace depends on the rows' contents and not on where they lie"""
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import NO_CONS, to_dev

    torch, prover = gpu
    airs_of, length, period, n_calls, n_access, log_big = [0, 1, 0], 2, 3, 37, 5, 24
    n = n_calls * period + 2
    ex = sref.Execution(n, seed=13, n_access=n_access)
    rows = [(4 * (i % period), ts, 4 * ((i + 1) % period), nts, acc) for i, (_, ts, _, nts, acc) in enumerate(ex.rows)]
    it = sref.state_log_interactions(n_access)
    parts = [[r for r in rows if airs_of[r[0] // 4] == air] for air in (0, 1)]
    small = [(sref.state_log(part, n_access, log_h=7), it) for part in parts]
    monty = [(om.to_monty(np.ascontiguousarray(cols)).reshape(cols.shape), it) for cols, it in small]
    calls = [(0, j * period, j * period + length) for j in range(n_calls)]
    layout, lists = dref.lists(small, [length], calls)
    assert layout[0] == (n_calls, [(0, 0), (1, 0)])
    places = np.sort(np.random.default_rng(24).permutation(1 << log_big)[:len(parts[1])])
    places[-1] = (1 << log_big) - 1  # the very last word of the trace is read
    big = torch.zeros((65, 1 << log_big), dtype=torch.int32, device="cuda")
    big[:, torch.from_numpy(places).cuda()] = torch.from_numpy(monty[1][0][:, :len(parts[1])].view(np.int32)).cuda()
    provers = [prover.Prover(65, *NO_CONS, num_queries=2, interactions=it) for _ in range(2)]
    t0 = to_dev(torch, small[0][0])
    seg = [(provers[0], t0.data_ptr(), 7), (provers[1], big.data_ptr(), log_big)]
    try:
        cells = [(1, 64, 0), (1, 0, 1), (0, 64, 2), (1, 63, 4)]
        want = dref.traces(monty, layout, lists, 0, cells, 64, 5)
        with aps.apply_calls(seg, calls, [length], direct=True) as direct, aps.apply_calls(seg, calls, [length]) as plain:
            got = outputs(torch, direct, [(0, cells, 64, 5)])[0]
            assert (got == want).all() and want[[0, 2, 4], :n_calls].any() and (got[3] == dref.FILL).all()
            assert (two_step(torch, plain, (0, cells, 64, 5))[[0, 1, 2, 4]] == got[[0, 1, 2, 4]]).all()
            assert direct.residual(1).rows == 1 and plain.source(0, 1).height == 64
    finally:
        for p in provers:
            p.close()


def test_statuses_and_refusals(gpu):
    from powdr_amd import apc_sources as aps
    from tests.test_bus_check_gpu import Segment

    # 11 and 12 as with flags 0
    host = sref.Execution(40, seed=2).airs()
    pos, _ = ref.where(host)
    p = next(i for i in range(1, 40) if pos[i][0] != pos[0][0])
    q = next(i for i in range(p + 1, 40) if pos[i][0] != pos[0][0])
    s = Segment(gpu, host)
    try:
        def status(cycles, calls, **kw):
            got = []
            for direct in (False, True):
                try:
                    aps.apply_calls(s.seg, calls, cycles, direct=direct, **kw).close()
                    got.append(None)
                except aps.ApcSourcesError as e:
                    got.append((e.status, e.info))
                assert aps.last_stats()["scratch_bytes"] == 0
            assert got[0] == got[1]
            return got[1]

        assert status([3, 2], [(0, 0, 3), (1, 5, 7), (0, 38, 41), (1, 41, 43)]) == (11, 2)
        assert status([3], [(0, 37, 40)]) is None
        assert status([1], [(0, 0, 1), (0, q, q + 1)]) == (12, q)
        assert status([1], [(0, 0, 1), (0, p, p + 1), (0, q, q + 1)]) == (12, p)
        assert status([1], [(0, 0, 1), (0, q, q + 1), (0, 40, 41)]) == (11, 2)
    finally:
        s.close()

    # status 2: the direct bound leaves the source matrices out; a run inside the bytes it names
    host, monty, calls = periodic_log(1025, 3)
    cycles = [4, 1]
    s = Segment(gpu, host)
    try:
        info = {}
        for direct in (False, True):
            with pytest.raises(aps.ApcSourcesError) as e:
                aps.apply_calls(s.seg, calls, cycles, scratch_bytes=1, direct=direct)
            assert e.value.status == 2 and aps.last_stats()["scratch_bytes"] == 0
            info[direct] = e.value.info
        with aps.apply_calls(s.seg, calls, cycles) as plain:
            assert plain.source_bytes > 0 and info[False] - info[True] >= plain.source_bytes
        with aps.apply_calls(s.seg, calls, cycles, scratch_bytes=info[True], direct=True) as direct:
            stats = aps.last_stats()
            assert 0 < stats["peak_bytes"] <= info[True] and stats["scratch_bytes"] == 0 and stats["source_bytes"] == 0
            assert stats["peak_bytes"] >= direct.index_bytes + direct.residual_bytes and direct.index_bytes >= 4 * direct.covered == 4 * 4 * 1025
            # every -1 of the new calls that needs a handle with calls; nothing is launched
            out = gpu[0].full((41 * 2048,), FILL_I32, dtype=gpu[0].int32, device="cuda")
            good = (0, [(0, 0, 0), (1, 40, 1)], out.data_ptr(), 2048, 41)

            def refused(*jobs):
                recs, keep = aps.trace_jobs(list(jobs))
                return aps.lib.pw_apc_sources_tracegen(direct._h, recs, len(jobs)) == -1

            assert refused((0, [(0, 41, 0)], *good[2:])) and refused((0, [(1, 0, 0), (1, 41, 1)], *good[2:]))  # col >= the AIR's width
            assert refused((0, [(4, 0, 0)], *good[2:])) and refused((2, [(0, 0, 0)], *good[2:]))  # instr >= cycle_count, apc >= n_apcs
            assert refused((0, good[1], out.data_ptr(), 1024, 41)) and refused((0, good[1], out.data_ptr(), 1536, 41))  # out_height < n_calls, no power of two
            assert refused((0, [(0, 0, 41)], *good[2:])) and refused((0, [(0, 0, 3), (1, 1, 3)], *good[2:])) and refused((0, good[1], out.data_ptr(), 2048, 0))
            assert refused(good, (1, [(0, 0, 0)], out.data_ptr() + 4 * 2048 * 40, 4, 1)) and refused((0, good[1], None, 2048, 41))
            assert aps.lib.pw_apc_sources_tracegen(None, None, 0) == -1
            with aps.apply_calls(s.seg, calls, cycles) as plain:  # a flags-0 handle
                recs, keep = aps.trace_jobs([good])
                assert aps.lib.pw_apc_sources_tracegen(plain._h, recs, 1) == -1
                with pytest.raises(ValueError, match="not direct"):
                    plain.apc_traces([good])
            gpu[0].cuda.synchronize()
            assert bool((out == FILL_I32).all())  # no refused call wrote a word
            direct.apc_traces([good])
            assert aps.tracegen_last_stats()["scratch_bytes"] == 0 and not bool((out.view(41, 2048)[:2] == FILL_I32).any())
        assert aps.last_stats()["scratch_bytes"] == 0 and aps.tracegen_last_stats()["scratch_bytes"] == 0
    finally:
        s.close()


def test_the_chained_execution_from_calls_to_apc_traces_without_source_matrices(gpu):
    """select_calls with registers -> apply_calls(direct=True) -> apc_traces on every cell of A's and B's instructions, against
    powdr_apc_tracegen_host_tables on the traces powdr_original_airs_expand makes of the selected records: the comparison
    tests/test_apc_sources_gpu.py makes for the two-step path"""
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
                aps.apply_calls(seg, chosen, apcs, min_log_height=2, direct=True) as got, aps.apply_calls(seg, chosen, apcs, min_log_height=2) as plain:
            assert [tuple(c) for c in chosen.calls] == want_calls and got.direct and got.source_bytes == 0 and got.index_bytes >= 4 * got.covered
            assert [tuple(l) for l in got.layout] == [tuple(l) for l in plain.layout] == ref.apply(host, cycles, want_calls, min_log_height=2)["layout"]
            block = [(int(ins["kind"]), int(ins["air_row"])) for ins in ex.table]
            jobs, outs, theirs = [], [], []
            for a, n_calls, height in ((0, 1, 4), (1, 31, 32)):
                instrs = block if a == 0 else block + [(k, row + ex.rbs[k]) for k, row in block]
                cells = [(i, col) for i, (k, _) in enumerate(instrs) for col in range(pc.WIDTHS[k])]
                outs.append(torch.full((len(cells) * height,), FILL_I32, dtype=torch.int32, device="cuda"))
                jobs.append((a, [(i, col, c) for c, (i, col) in enumerate(cells)], outs[-1].data_ptr(), height, len(cells)))
                sel_seg = selected[a][0]
                h_airs = (abi.OriginalAir * len(kinds))(*[abi.OriginalAir(pc.WIDTHS[k], 1 << sel_seg[air][2], sel_seg[air][1], (a + 1) * ex.rbs[k])
                                                          for air, k in enumerate(kinds)])
                subs = [(kinds.index(instrs[i][0]), col, instrs[i][1], c) for c, (i, col) in enumerate(cells)]
                theirs.append(tracegen(torch, h_airs, len(kinds), subs, height, len(cells), n_calls))
            torch.cuda.synchronize()
            got.apc_traces(jobs)  # both APCs: one call
            assert aps.tracegen_last_stats()["jobs"] == 2
            for out, want, (a, cells, _, height, width) in zip(outs, theirs, jobs):
                mine = out.cpu().numpy().view(np.uint32).reshape(width, height)
                assert (mine == want).all() and mine[:, :plain.layout[a].n_calls].any(), a
            # the buses of the residual segment: what the flags-0 handle's residual segment reports
            mine_s, mine_t = prover.check_segment_buses(got.residual_segment(seg), tuple_cap=1 << 16)
            their_s, their_t = prover.check_segment_buses(plain.residual_segment(seg), tuple_cap=1 << 16)
            assert mine_s == their_s and mine_t == their_t and len(mine_s) > 3
        assert aps.last_stats()["scratch_bytes"] == 0 and aps.tracegen_last_stats()["scratch_bytes"] == 0
    finally:
        for group in [seg] + [v[0] for v in selected.values()]:
            for p, _, _ in group:
                p.close()
