"""pw_execution_states_from_traces on the GPU against the restatement of tests/_execution_states_ref.py: the register
table, the pcs and the time keys word for word, and every status with the info the restatement names."""
import numpy as np
import pytest

from tests import _empirical_ref as eref
from tests import _execution_states_ref as sref

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 63, 64, 65, 1025, 2**16 + 1]


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def device_states(gpu, airs, regs, final_pc, **kw):
    """-> (pcs, table, time keys, stats) of the device for host AIRs"""
    from powdr_amd import execution_states as es
    from tests.test_bus_check_gpu import Segment

    s = Segment(gpu, airs)
    try:
        with es.states_from_traces(s.seg, regs, final_pc, **kw) as got:
            assert got.n_regs == len(list(regs)) and got.bytes > 0 and got.d_pcs
            return got.pcs().tolist(), got.regs(), got.time_keys, dict(es.last_stats(), sends=got.sends, n_states=got.n_states)
    finally:
        s.close()


def same(gpu, airs, regs, final_pc, **kw):
    want = sref.states(airs, regs, final_pc, **{k: v for k, v in kw.items() if k != "scratch_bytes"})
    pcs, table, keys, stats = device_states(gpu, airs, regs, final_pc, **kw)
    assert pcs == want["pcs"] and keys == want["time_keys"] and stats["n_states"] == len(want["pcs"])
    assert table.shape == want["regs"].shape and (table == want["regs"]).all(), np.argwhere(table != want["regs"])[:5]
    assert stats["sends"] == want["sends"] and stats["scratch_bytes"] == 0
    return want, table, stats


def status_of(gpu, airs, regs, final_pc, **kw):
    """the device's (status, info), which must be the restatement's"""
    from powdr_amd import execution_states as es

    with pytest.raises(sref.Status) as want:
        sref.states(airs, regs, final_pc, **kw)
    with pytest.raises(es.ExecutionStatesError) as got:
        device_states(gpu, airs, regs, final_pc, **kw)
    assert (got.value.status, got.value.info) == (want.value.status, want.value.info)
    assert es.last_stats()["scratch_bytes"] == 0  # (a status raised after the stages allocated: 8, 9, 10)
    return got.value


@pytest.mark.parametrize("n", SIZES)
def test_state_logs_permuted_across_two_airs(gpu, n):
    """random accesses, a quarter of them to address space 2 at the registers' own pointers"""
    ex = sref.Execution(n, seed=n + 5)
    regs = sorted(ex.accessed, reverse=True)  # (rows in the caller's order, not the registers')
    want, _, _ = same(gpu, ex.airs(), regs, ex.final_pc, segments=[3, 3])
    assert (want["regs"] == ex.truth[regs]).all() and all(k >> 32 == 3 for k in want["time_keys"])
    if n:
        same(gpu, ex.airs(), range(ex.n_regs), ex.final_pc, initial_regs=ex.initial)


def test_the_tile_edges_of_the_fill(gpu):
    from powdr_amd import execution_states as es

    T = es.last_stats()["fill_tile"]
    assert T >= 64
    n, late = 3 * T + 5, (2 * T + 149) // 50 * 50  # a multiple of 50 past two tiles
    rng = np.random.default_rng(8)
    words = rng.integers(0, 1 << 32, size=(3, n)).tolist()

    def plan(i):
        todo = [(1, 0, words[0][i])]  # x0 of this log: a write at every position
        if i % T in (T - 2, T - 1, 0, 1):
            todo.append((1, 1, words[1][i]))  # writes seen from k T - 1, k T, k T + 1 and k T + 2 on only
        if i == n - 1:
            todo.append((1, 2, 77))  # the only write is the last instruction's
        if i == 7:
            todo.append((1, 3, None))  # read, never changed
        if i >= late and i % 50 == 0:
            todo.append((1, 4, words[2][i]))  # first touched after more than two tiles
        return todo

    ex = sref.Execution(n, seed=1, n_regs=6, n_access=5, plan=plan)
    assert ex.accessed == {0, 1, 2, 3, 4}
    want, table, stats = same(gpu, ex.airs(), range(6), ex.final_pc, initial_regs=ex.initial)
    assert (table == ex.truth).all() and stats["kept"] == stats["sends"]
    assert (table[2, :-1] == ex.initial[2]).all() and table[2, -1] == 77 and (table[3] == ex.initial[3]).all()
    assert (table[4, :late + 1] == ex.initial[4]).all() and table[4, late + 1] != ex.initial[4] and (table[5] == ex.initial[5]).all()
    for regs in ([1], [4, 1], [2, 0, 1], [3, 2, 1, 0]):  # every alignment of a row's first word
        same(gpu, ex.airs(), regs, ex.final_pc)


def test_two_accesses_of_one_instruction_to_one_register(gpu):
    def plan(i):
        if i % 3 == 0:
            return [(1, 3, None), (1, 2, None), (1, 3, 1000 + i)]  # ADD x3 = x3 + x2: reads x3, then writes it
        if i % 3 == 1:
            return [(1, 2, 5 * i), (1, 2, 7 * i)]  # two writes: the later one stays
        return []

    ex = sref.Execution(200, seed=2, plan=plan)
    want, table, stats = same(gpu, ex.airs(), [2, 3], ex.final_pc)
    assert (table == ex.truth[[2, 3]]).all() and stats["kept"] < stats["sends"] and table[0, 2] == 7


def test_a_register_that_is_never_accessed(gpu):
    ex = sref.Execution(100, seed=4, plan=lambda i: [(1, i % 3, i)])
    e = status_of(gpu, ex.airs(), [1, 5, 4], ex.final_pc)
    assert (e.status, e.info) == (9, 4) and "register 4" in str(e)
    want, table, _ = same(gpu, ex.airs(), [1, 5, 4], ex.final_pc, initial_regs=[ex.initial[1], 55, 44])
    assert (table[1] == 55).all() and (table[2] == 44).all()
    e = status_of(gpu, ex.airs(), [1, 5, 0], ex.final_pc, initial_regs=[ex.initial[1], 55, ex.initial[0] ^ 4])
    assert (e.status, e.info) == (10, 0)


def test_status_8_names_the_smallest_witness(gpu):
    ex = sref.Execution(40, seed=6, n_regs=3, plan=lambda i: [(1, i % 3, i), (1, (i + 1) % 3, None)])
    it = sref.state_log_interactions(2)
    c0, c1 = sref.HEAD, sref.HEAD + sref.PER_ACCESS
    base = sref.state_log(ex.rows, 2)

    def tampered(change):
        cols = base.copy()
        change(cols)
        return [(sref.state_log(ex.rows[:1], 2)[:, :2] * 0, it), (cols, it)]  # (an AIR without an active row in front: air 1 is named)

    def twice(cols):  # row 11 one tick after row 10: its access 0 sends to x2 at the time of row 10's access 1
        cols[2, 11] = cols[2, 10] + 1

    def early(cols):  # a row off the bridge whose send lies before the first instruction
        cols[:, 50] = cols[:, 5]
        cols[0, 50], cols[2, 50] = 0, 10

    causes = {"multiplicity": (lambda cols: cols.__setitem__((c1, 9), 2), (1, 4, 9)), "pointer": (lambda cols: cols.__setitem__((c0 + 2, 20), 5), (1, 2, 20)),
              "data word": (lambda cols: cols.__setitem__((c1 + 8, 30), 256), (1, 5, 30)), "twice": (twice, (1, 3, 11)), "early": (early, (1, 3, 50))}
    for name, (change, witness) in causes.items():
        e = status_of(gpu, tampered(change), range(3), ex.final_pc)
        assert e.status == 8 and e.info == sref.pack_witness(*witness), (name, e.info)
    e = status_of(gpu, tampered(lambda cols: (early(cols), cols.__setitem__((c1 + 8, 30), 256))), range(3), ex.final_pc)
    assert e.info == sref.pack_witness(1, 3, 50) and "air 1, interaction 3, row 50" in str(e)  # the smallest of two


def test_status_2_and_the_bytes_it_names(gpu):
    from powdr_amd import execution_states as es

    ex = sref.Execution(3000, seed=9)
    with pytest.raises(es.ExecutionStatesError) as e:
        device_states(gpu, ex.airs(), range(6), ex.final_pc, initial_regs=ex.initial, scratch_bytes=1)
    assert e.value.status == 2 and e.value.info > 1 and "bytes needed" in str(e.value) and es.last_stats()["scratch_bytes"] == 0
    _, _, stats = same(gpu, ex.airs(), range(6), ex.final_pc, initial_regs=ex.initial, scratch_bytes=e.value.info)
    assert 0 < stats["peak_bytes"] <= e.value.info
    with pytest.raises(es.ExecutionStatesError) as again:
        device_states(gpu, ex.airs(), range(6), ex.final_pc, initial_regs=ex.initial, scratch_bytes=e.value.info - 1)
    assert (again.value.status, again.value.info) == (2, e.value.info)


def test_two_runs_give_the_same_bytes(gpu):
    ex = sref.Execution(5000, seed=12)
    runs = [device_states(gpu, ex.airs(), range(6), ex.final_pc, initial_regs=ex.initial) for _ in range(2)]
    assert runs[0][0] == runs[1][0] and runs[0][2] == runs[1][2] and runs[0][1].tobytes() == runs[1][1].tobytes()


def test_refusals_that_need_a_prover(gpu):
    ex = sref.Execution(8, seed=1)
    short = [(eref.block_log([(0, 5, [0])], 1), eref.block_log_interactions(bus=1))]  # two arguments on the memory bus
    with pytest.raises(ValueError, match="malformed"):
        device_states(gpu, ex.airs() + short, [1], ex.final_pc)
    with pytest.raises(ValueError, match="malformed"):
        device_states(gpu, ex.airs(), [1], ex.final_pc, segments=[0, 1])
    with pytest.raises(ValueError, match="malformed"):
        device_states(gpu, ex.airs(), [1, 1], ex.final_pc)


def test_the_chained_execution(gpu):
    from powdr_amd import execution_states as es
    from tests import _chained_vm as vm
    from tests.test_empirical_gpu import device_airs, host_airs

    ex = vm.Execution(64, seed=3)
    want = sref.states(host_airs(ex, ex.rec), range(1, 8), ex.end[0])
    seg, keep, _ = device_airs(gpu, ex.table, ex.rec, 64)
    try:
        with es.states_from_traces(seg, range(1, 8), ex.end[0]) as got:
            assert got.pcs().tolist() == want["pcs"] and got.time_keys == want["time_keys"] and (got.regs() == want["regs"]).all()
            assert got.sends == want["sends"] and [int(got.regs()[k, -1]) for k in range(7)] == [ex.final[(1, 4 * r)][0] for r in range(1, 8)]
    finally:
        for p, _, _ in seg:
            p.close()
