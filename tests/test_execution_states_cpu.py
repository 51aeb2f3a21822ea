"""The states of an execution from its traces without a GPU: the restatement of tests/_execution_states_ref.py on §5j's
chained execution and on the state log's own ground truth, and every refusal of the two new entry points that needs no GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import _execution_states_ref as sref


@pytest.fixture(scope="module")
def chained():
    from tests import _chained_vm as vm
    from tests.test_empirical_gpu import host_airs

    ex = vm.Execution(16, seed=3)
    return vm, ex, sref.states(host_airs(ex, ex.rec), range(1, 8), ex.end[0])


def test_the_chained_execution_gives_initial_and_final(chained):
    vm, ex, got = chained
    n = len(vm.BLOCK)
    assert got["regs"].shape == (7, 16 * n + 1) and len(got["time_keys"]) == 16 * n
    for k, reg in enumerate(range(1, 8)):
        assert int(got["regs"][k, 0]) == ex.initial[(1, 4 * reg)][0] and int(got["regs"][k, -1]) == ex.final[(1, 4 * reg)][0], reg
    assert got["pcs"] == [vm.START_PC + 4 * i for i in range(n)] * 16 + [ex.end[0]]
    assert got["time_keys"] == sorted(got["time_keys"]) and got["time_keys"][0] == ex.start[1]


def test_x2_counts_the_calls_and_x1_steps_by_4(chained):
    vm, ex, got = chained
    n = len(vm.BLOCK)
    starts = got["regs"][:, ::n].astype(np.int64)  # the registers at the 17 block starts
    assert (np.diff(starts[1]) % (1 << 32) == 1).all() and (np.diff(starts[0]) % (1 << 32) == 4).all()
    assert 0 not in got["accessed"] and got["accessed"] == set(range(1, 8))


def test_x0_is_never_accessed(chained):
    from tests.test_empirical_gpu import host_airs

    vm, ex, _ = chained
    with pytest.raises(sref.Status) as e:
        sref.states(host_airs(ex, ex.rec), [0, 1], ex.end[0])
    assert (e.value.status, e.value.info) == (9, 0)
    got = sref.states(host_airs(ex, ex.rec), [0, 2], ex.end[0], initial_regs=[0, ex.initial[(1, 8)][0]])
    assert not got["regs"][0].any()
    with pytest.raises(sref.Status) as e:
        sref.states(host_airs(ex, ex.rec), [0, 2], ex.end[0], initial_regs=[0, ex.initial[(1, 8)][0] ^ 1])
    assert (e.value.status, e.value.info) == (10, 2)


@pytest.mark.parametrize("n", [0, 1, 2, 65, 1025])
def test_the_state_logs_ground_truth(n):
    ex = sref.Execution(n, seed=n)
    regs = sorted(ex.accessed)
    got = sref.states(ex.airs(), regs, ex.final_pc)
    assert got["pcs"] == ex.pcs and (got["regs"] == ex.truth[regs]).all()
    everything = sref.states(ex.airs(split=False), range(ex.n_regs), ex.final_pc, initial_regs=ex.initial)
    assert (everything["regs"] == ex.truth).all() and everything["time_keys"] == [1000 + 3 * i for i in range(n)]


def test_every_refusal_that_needs_no_gpu():
    from powdr_amd import apc_calls as ac
    from powdr_amd import execution_states as es
    from powdr_amd import prover

    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    recs = (prover.PwSegmentAir * 2)()
    regs = (C.c_uint32 * 3)(1, 2, 3)

    def states(recs=recs, seg=None, n_airs=0, bus=0, memory_bus=1, step=4, regs=regs, n_regs=3, out=C.byref(out), status=C.byref(status), info=C.byref(info)):
        return es.lib.pw_execution_states_from_traces(recs, seg, n_airs, bus, memory_bus, 0, 1, step, regs, n_regs, None, 0, out, status, info)

    for null in ("out", "status", "info", "regs"):
        assert states(**{null: None}) == -1, null
    assert states(recs=None, n_airs=2) == -1
    assert states(step=0) == -1
    assert states(regs=(C.c_uint32 * 3)(1, 2, 1)) == -1  # one register twice
    assert states(regs=(C.c_uint32 * 3)(1, 2, sref.P // 4 + 1)) == -1  # a pointer that is no field element
    assert states(bus=sref.P) == -1 and states(memory_bus=sref.P) == -1
    assert states(n_airs=2, seg=(C.c_uint32 * 2)(0, 1)) == -1  # two segment numbers
    assert states(n_airs=2) == -1  # (a NULL prover: refused with the AIR list)

    good = ac.tables([ac.Apc(0, 2, 1, [(ac.Pc(0), ac.Number(0)), (ac.RegisterLimb(1, 5, 3), ac.Number(7))])])
    po = C.c_void_p()

    def calls(tabs=good, recs=recs, seg=None, n_airs=0, bus=0, memory_bus=1, step=4, n_regs=32, limb_bits=8, out=C.byref(po), status=C.byref(status), info=C.byref(info)):
        return ac.lib.pw_apc_calls_from_traces_registers(recs, seg, n_airs, bus, memory_bus, 0, 1, step, n_regs, limb_bits, None, *tabs, 0, out, status, info)

    for null in ("out", "status", "info"):
        assert calls(**{null: None}) == -1, null
    assert calls(recs=None, n_airs=2) == -1 and calls(n_airs=2) == -1
    assert calls(step=0) == -1 and calls(bus=sref.P) == -1 and calls(memory_bus=sref.P) == -1
    assert calls(n_airs=2, seg=(C.c_uint32 * 2)(0, 1)) == -1
    assert calls(n_regs=5) == -1  # reg >= n_regs
    assert calls(limb_bits=16) == -1 and calls(limb_bits=0) == -1  # limb * limb_bits >= 32; no limb width
    assert calls(tabs=ac.tables([ac.Apc(0, 0, 1)])) == -1  # cycle_count == 0
    assert calls(tabs=ac.tables([ac.Apc(0, 1, 1, [(ac.RegisterLimb(0, sref.P // 4 + 1, 0), ac.Number(0))])]), n_regs=sref.P) == -1  # no field element


def test_without_registers_select_calls_raises_as_before():
    from powdr_amd import apc_calls as ac

    with pytest.raises(ValueError, match="final_pc"):
        ac.select_calls([(type("P", (), {"_h": None})(), 0, 1)], [ac.Apc(0, 1, 1)])
    with pytest.raises(ValueError, match="trace route only"):
        ac.select_calls([0, 4], [ac.Apc(0, 1, 1)], registers=dict(n_regs=32))
    assert ac.STATUS[8] and ac.STATUS[9] and ac.STATUS[10]
    e = ac.ApcCallsError(8, (1 << 46) | (2 << 26) | 3)
    assert "air 1, interaction 2, row 3" in str(e) and "register 5" in str(ac.ApcCallsError(9, 5))
