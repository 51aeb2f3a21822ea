"""pw-stark v1 + public values on the device: AIRs whose constraints read public values, in segment proofs (magic PWS6)
next to plain, preprocessed, row-aware and streamed AIRs, on every expression path; the mock prover against a twin with the values baked
in as constants; the refusals; and three chained segments of one execution whose public connectors the chain verifier links."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _chained_vm as vm
from tests.test_preprocessed_segment_gpu import NO_INTER, RAMP_CONS, RAMP_INTER, cons_tables, ramp_fixed, ramp_trace, to_dev
from tests.test_segment_proof import SPEC, synthetic_airs
from tests.test_transition_segment_gpu import fib_trace

pytestmark = pytest.mark.gpu
P = om.P
PA, PC, ADD, SUB, MUL, NEG = 0, 1, 2, 3, 4, 5
MAGIC3, MAGIC4, MAGIC5, MAGIC6 = 0x33535750, 0x34535750, 0x35535750, 0x36535750
NQ = 5


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def prove(prover, airs, logup):
    return prover.prove_segment([(p, t.data_ptr(), h) for p, t, h in airs], logup=logup)


def close(airs):
    for p, _, _ in airs:
        p.close()


# ---- AIRs ---------------------------------------------------------------------------------------------------------------------------
def fib_public_program(consts=None):
    """[a, b]: is_first_row (a - pv0), is_first_row (b - pv1), is_last_row (b - pv2), is_transition (a' - b), is_transition (b' - a - b);
    consts: the twin — the three values as PUSH_CONST"""
    from powdr_amd.prover import row_operands

    r = row_operands(2)
    pv = (lambda k: [PC, int(consts[k])]) if consts is not None else (lambda k: [PA, r.public(k)])
    return cons_tables([[PA, r.is_first_row, PA, 0, *pv(0), SUB, MUL],
                        [PA, r.is_first_row, PA, 1, *pv(1), SUB, MUL],
                        [PA, r.is_last_row, PA, 1, *pv(2), SUB, MUL],
                        [PA, r.is_transition, PA, r.next(0), PA, 1, SUB, MUL],
                        [PA, r.is_transition, PA, r.next(1), PA, 0, SUB, PA, 1, SUB, MUL]])


def fib_public(t):
    return np.array([t[0, 0], t[1, 0], t[1, -1]], np.uint32)


WIDE_W, WIDE_NP = 40, 70


def wide_program():
    """the public-only AIR: 40 columns, 70 public values, constraint k = c_i (c_j - pv_k) with i = k mod 8 and j = 8 + k div 8 —
    every (i, j) occurs once, so every public value is pinned by its own cells (wide_trace) and no two of them are equal"""
    from powdr_amd.prover import row_operands

    r = row_operands(WIDE_W)
    return cons_tables([[PA, k % 8, PA, 8 + k // 8, PA, r.public(k), SUB, MUL] for k in range(WIDE_NP)])


def wide_trace(h, seed):
    """columns 0 .. 7: column i is non-zero exactly on the rows = i mod 8; columns 8 .. 39: c_j[row] = u[j, row mod 8] -> (trace, the
    public values u[8 + k div 8, k mod 8])"""
    rng = np.random.default_rng([seed, h])
    H = 1 << h
    row = np.arange(H)
    t = np.zeros((WIDE_W, H), np.uint32)
    for i in range(8):
        t[i] = np.where(row % 8 == i, rng.integers(1, P, H), 0)
    u = rng.integers(0, P, (WIDE_W, 8)).astype(np.uint32)
    for j in range(8, WIDE_W):
        t[j] = u[j, row % 8]
    return t, np.array([u[8 + k // 8, k % 8] for k in range(WIDE_NP)], np.uint32)


# ---- 1. a row-aware AIR with public values ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logup", [False, True], ids=["constraints", "logup"])
@pytest.mark.parametrize("h", [1, 4, 10])
def test_fibonacci_with_public_values(gpu, h, logup):
    torch, prover = gpu
    t = fib_trace(h, 3, 5)
    cons, it = fib_public_program(), NO_INTER if logup else None
    pr = prover.Prover(2, *cons, num_queries=6, pow_bits=2, interactions=it, n_public=3)
    assert pr.row_flags == 3 and pr.max_constraint_degree() == 2
    true = fib_public(t)
    pr.set_public_values(true)
    d = to_dev(torch, t)
    assert pr.check_constraints(d.data_ptr(), h)[0] == 0
    pf = prove(prover, [(pr, d, h)], logup)
    assert pf[0] == MAGIC6 and (pf[9:12] == true).all()  # right after the header: 5 + 4 words
    desc = [(2, h, *cons, it)]
    assert prover.verify_segment(desc, pf, 6, 2, logup, public=[3])[0] == 0
    assert prover.verify_segment(desc, pf, 6, 2, logup, public=[true])[0] == 0
    assert (prover.segment_public_values(desc, pf, [3], 0) == true).all()
    wrong = true.copy()
    wrong[2] = (int(wrong[2]) + 1) % P
    assert prover.verify_segment(desc, pf, 6, 2, logup, public=[wrong])[0] == 17
    # the verifiers without public values: not their magic
    assert prover.verify_segment(desc, pf, 6, 2, logup, public=[None])[0] == 15  # (the operands are past the row layout)
    twin = [(2, h, *fib_public_program(true), it)]
    assert prover.verify_segment(twin, pf, 6, 2, logup, transition=True)[0] == 1
    # the carried pv2 changed: the transcript and the identity at zeta read it
    bad = pf.copy()
    bad[11] = (int(bad[11]) + 1) % P
    assert prover.verify_segment(desc, bad, 6, 2, logup, public=[3])[0] != 0
    assert prover.verify_segment(desc, bad, 6, 2, logup, public=[true])[0] == 17
    pr.close()


# ---- 2. public-only AIRs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [6, 16])
def test_public_only_air(gpu, monkeypatch, h):
    torch, prover = gpu
    cons = wide_program()
    t, true = wide_trace(h, 1)
    assert len(set(true.tolist())) == WIDE_NP
    pr = prover.Prover(WIDE_W, *cons, num_queries=NQ, pow_bits=2, interactions=NO_INTER, n_public=WIDE_NP)
    assert pr.row_flags == 0 and pr.max_constraint_degree() == 2
    syn = synthetic_airs([("T0", 30)])[0]
    plain = prover.Prover(syn[1], syn[3], syn[4], num_queries=NQ, pow_bits=2, interactions=syn[5])
    d, ds = to_dev(torch, t), to_dev(torch, syn[0])
    pr.set_public_values(true)
    assert pr.check_constraints(d.data_ptr(), h)[0] == 0
    airs = [(pr, d, h), (plain, ds, syn[2])]
    descs = [(WIDE_W, h, *cons, NO_INTER), (syn[1], syn[2], syn[3], syn[4], syn[5])]
    pf = prove(prover, airs, True)
    assert pf[0] == MAGIC6 and prover.segment_last_modes() == [(0, False), (0, False)]
    assert prover.verify_segment(descs, pf, NQ, 2, True, public=[true, None])[0] == 0
    assert (prover.segment_public_values(descs, pf, [WIDE_NP, None], 0) == true).all()
    # never streamed, whatever the other AIRs do; the same words
    assert syn[2] >= 3
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS", "1")
    assert (prove(prover, airs, True) == pf).all()
    assert prover.segment_last_modes() == [(0, False), (1, False)]
    monkeypatch.delenv("POWDR_STREAM_LOG_BLOCKS")
    # every value is read at its own index: one of them off by one breaks exactly its constraint, on the rows that pin it
    for k in (0, 63, 64, WIDE_NP - 1):
        wrong = true.copy()
        wrong[k] = (int(wrong[k]) + 1) % P
        pr.set_public_values(wrong)
        n, row, c = pr.check_constraints(d.data_ptr(), h)
        assert (n, row, c) == ((1 << h) // 8, k % 8, k)
    if h == 6:
        assert prover.verify_segment(descs, prove(prover, airs, True), NQ, 2, True, public=[WIDE_NP, None])[0] == (1 << 8) | 2
    close(airs)


# ---- 3. every path, the same words ------------------------------------------------------------------------------------------------------
FIB_H, WIDE_H, RAMP_H = 6, 6, 7
CONNECTOR_STATES = ((0x200000, 1000), (0x200028, 1234))


def mixed_segment(torch, prover, logup, fib_start=(3, 5), states=CONNECTOR_STATES):
    """-> (airs [(Prover, trace, h)], descriptions, keys, public): Fibonacci with public values (row-aware), the public-only AIR, the
    synthetic AIRs, a plain preprocessed AIR and the public connector; every public value set"""
    from powdr_amd import system_airs as sa

    airs, descs, keys, public = [], [], [], []
    it = lambda x: x if logup else None
    ft = fib_trace(FIB_H, *fib_start)
    fc = fib_public_program()
    airs.append((prover.Prover(2, *fc, num_queries=NQ, pow_bits=2, interactions=it(NO_INTER), n_public=3), to_dev(torch, ft), FIB_H))
    descs.append((2, FIB_H, *fc, it(NO_INTER)))
    keys.append(None)
    public.append(fib_public(ft))
    wt, wv = wide_trace(WIDE_H, 2)
    wc = wide_program()
    airs.append((prover.Prover(WIDE_W, *wc, num_queries=NQ, pow_bits=2, interactions=it(NO_INTER), n_public=WIDE_NP), to_dev(torch, wt), WIDE_H))
    descs.append((WIDE_W, WIDE_H, *wc, it(NO_INTER)))
    keys.append(None)
    public.append(wv)
    for a in synthetic_airs(SPEC):
        airs.append((prover.Prover(a[1], a[3], a[4], num_queries=NQ, pow_bits=2, interactions=it(a[5])), to_dev(torch, a[0]), a[2]))
        descs.append((a[1], a[2], a[3], a[4], it(a[5])))
        keys.append(None)
        public.append(None)
    rp = prover.Prover(2, *RAMP_CONS, num_queries=NQ, pow_bits=2, interactions=it(RAMP_INTER), preprocessed=(to_dev(torch, ramp_fixed(RAMP_H)), 2, RAMP_H))
    airs.append((rp, to_dev(torch, ramp_trace(RAMP_H, 5)), RAMP_H))
    descs.append((2, RAMP_H, *RAMP_CONS, it(RAMP_INTER)))
    keys.append((2, rp.preprocessed_root()))
    public.append(None)
    con = sa.connector_air(public=True)
    torch.cuda.synchronize()
    cp = prover.Prover(2, *con.cons, num_queries=NQ, pow_bits=2, interactions=it(con.inter), preprocessed=(con.fixed_table(), 1, 1), n_public=4)
    (pc0, ts0), (pc1, ts1) = states
    airs.append((cp, to_dev(torch, np.array([pc0, pc1, ts0, ts1], np.uint32)), 1))
    descs.append((2, 1, *con.cons, it(con.inter)))
    keys.append((1, cp.preprocessed_root()))
    public.append(np.array([pc0, ts0, pc1, ts1], np.uint32))
    for (p, _, _), v in zip(airs, public):
        if v is not None:
            p.set_public_values(v)
    return airs, descs, keys, public


@pytest.mark.parametrize("logup", [False, True], ids=["constraints", "logup"])
def test_mixed_segment_on_every_path(gpu, monkeypatch, logup):
    torch, prover = gpu
    airs, descs, keys, public = mixed_segment(torch, prover, logup)
    assert [p.row_flags for p, _, _ in airs] == [3] + [0] * (len(airs) - 1)
    for p, t, h in airs:
        assert p.check_constraints(t.data_ptr(), h)[0] == 0
    pf = prove(prover, airs, logup)
    assert pf[0] == MAGIC6
    counts = [None if v is None else len(v) for v in public]
    assert prover.verify_segment(descs, pf, NQ, 2, logup, preprocessed=keys, public=public)[0] == 0
    assert prover.verify_segment(descs, pf, NQ, 2, logup, preprocessed=keys, public=counts)[0] == 0
    assert prover.verify_segment(descs, pf, NQ, 2, logup, preprocessed=keys, transition=True)[0] == 15
    for a, v in enumerate(public):
        if v is not None:
            assert (prover.segment_public_values(descs, pf, counts, a) == v).all()
    monkeypatch.setenv("POWDR_SEGMENT_STREAMS", "0")
    assert (prove(prover, airs, logup) == pf).all()
    monkeypatch.delenv("POWDR_SEGMENT_STREAMS")
    variants = [("POWDR_QUOTIENT_XBC", "0")] + ([("POWDR_LOGUP_INTERPRET", "1")] if logup else [])
    for name, value in variants:  # read at creation
        monkeypatch.setenv(name, value)
        other = mixed_segment(torch, prover, logup)[0]
        monkeypatch.delenv(name)
        if name == "POWDR_LOGUP_INTERPRET":
            assert other[-1][0].logup_path() == 1
        assert (prove(prover, other, logup) == pf).all(), name
        close(other)
    prover.specialise_all([p for p, _, _ in airs])
    pub_airs = [a for a, v in enumerate(public) if v is not None]
    for a in pub_airs:
        st = airs[a][0].specialised()
        assert st["state"] == 1 and st["kernels"] >= 1
    assert (prove(prover, airs, logup) == pf).all()
    # other values on the same specialised provers: proven and verified without a recompilation (the code never held the values)
    before = prover.jit_cache_stats()
    ft = fib_trace(FIB_H, 11, 2)
    airs[0] = (airs[0][0], to_dev(torch, ft), FIB_H)
    public[0] = fib_public(ft)
    airs[0][0].set_public_values(public[0])
    (pc0, ts0), (pc1, ts1) = (0x200028, 1234), (0x200050, 1500)
    airs[-1] = (airs[-1][0], to_dev(torch, np.array([pc0, pc1, ts0, ts1], np.uint32)), 1)
    public[-1] = np.array([pc0, ts0, pc1, ts1], np.uint32)
    airs[-1][0].set_public_values(public[-1])
    pf2 = prove(prover, airs, logup)
    assert prover.verify_segment(descs, pf2, NQ, 2, logup, preprocessed=keys, public=public)[0] == 0
    assert prover.jit_cache_stats() == before
    fresh = mixed_segment(torch, prover, logup, fib_start=(11, 2), states=((pc0, ts0), (pc1, ts1)))[0]  # the interpreter agrees
    assert (prove(prover, fresh, logup) == pf2).all()
    close(fresh)
    close(airs)


# ---- 4. no change without public values -------------------------------------------------------------------------------------------------
def public_entry_prover(prover, width, bc, sp, interactions=None, preprocessed=None, n_public=0):
    """a Prover made by pw_prover_create_public whatever n_public is (Prover itself keeps the existing entries for n_public = 0)"""
    bc = np.ascontiguousarray(bc, dtype=np.uint32)
    sp = np.ascontiguousarray(sp, dtype=np.uint32).reshape(-1, 2)
    tables, keep = prover._interaction_tables(interactions)
    t, pw_, lh = preprocessed if preprocessed is not None else (None, 0, 0)
    cfg = prover.PwStarkConfig(NQ, 2)
    p = prover.Prover.__new__(prover.Prover)
    p.width, p.pre_width, p.n_public = width, pw_, n_public
    p._h = prover.lib.pw_prover_create_public(C.byref(cfg), width, pw_, lh, t.data_ptr() if t is not None else None, n_public, prover._vp(bc), len(bc),
                                             prover._vp(sp), len(sp), *tables)
    assert p._h
    return p


def test_without_public_values_the_new_entry_proves_todays_words(gpu):
    from tests.test_transition_segment_gpu import ACC_H, accum_program, accum_trace
    from tests.test_transition_segment_gpu import fib_program

    torch, prover = gpu
    for logup in (False, True):
        it = lambda x: x if logup else None
        syn = synthetic_airs(SPEC)
        want = sm.prove_segment(syn, num_queries=NQ, pow_bits=2, logup=logup)
        assert want[0] == MAGIC3
        ps = [(public_entry_prover(prover, a[1], a[3], a[4], it(a[5])), to_dev(torch, a[0]), a[2]) for a in syn]
        assert (prove(prover, ps, logup) == want).all()
        close(ps)
        # row-aware (with and without a fixed matrix), preprocessed and plain AIRs in one segment: the PWS5 words of the existing entries
        ft = fib_trace(FIB_H)
        parts = [(2, fib_program(int(ft[1, -1])), NO_INTER, None, ft, FIB_H, True),
                 (2, accum_program(), RAMP_INTER, (ramp_fixed(ACC_H), 2, ACC_H), accum_trace(ACC_H, 3), ACC_H, True),
                 (2, RAMP_CONS, RAMP_INTER, (ramp_fixed(RAMP_H), 2, RAMP_H), ramp_trace(RAMP_H, 5), RAMP_H, False),
                 (syn[0][1], (syn[0][3], syn[0][4]), syn[0][5], None, syn[0][0], syn[0][2], False)]
        got = []
        for new in (False, True):
            airs = []
            for w, cons, inter, fixed, t, h, transition in parts:
                pre = None if fixed is None else (to_dev(torch, fixed[0]), fixed[1], fixed[2])
                torch.cuda.synchronize()
                p = (public_entry_prover(prover, w, *cons, it(inter), pre) if new else
                     prover.Prover(w, *cons, num_queries=NQ, pow_bits=2, interactions=it(inter), preprocessed=pre, transition=transition))
                airs.append((p, to_dev(torch, t), h))
            assert [p.row_flags for p, _, _ in airs] == [3, 3, 0, 0]
            got.append(prove(prover, airs, logup))
            close(airs)
        assert got[0][0] == MAGIC5 and len(got[0]) == len(got[1]) and (got[0] == got[1]).all()
    # a preprocessed AIR alone: PWS4
    rp = public_entry_prover(prover, 2, *RAMP_CONS, RAMP_INTER, (to_dev(torch, ramp_fixed(RAMP_H)), 2, RAMP_H))
    old = prover.Prover(2, *RAMP_CONS, num_queries=NQ, pow_bits=2, interactions=RAMP_INTER, preprocessed=(to_dev(torch, ramp_fixed(RAMP_H)), 2, RAMP_H))
    sq = to_dev(torch, ramp_trace(RAMP_H, 1))
    a, b = prove(prover, [(rp, sq, RAMP_H)], True), prove(prover, [(old, sq, RAMP_H)], True)
    assert a[0] == MAGIC4 and (a == b).all()
    rp.close()
    old.close()


# ---- 5. the mock prover against a twin with the values baked in --------------------------------------------------------------------------
def test_mock_prover_matches_its_twin_with_constants(gpu):
    torch, prover = gpu
    h = 6
    t0 = fib_trace(h, 3, 5)
    true = fib_public(t0)
    cons = fib_public_program()
    pr = prover.Prover(2, *cons, num_queries=6, n_public=3)
    pr.set_public_values(true)
    twin = prover.Prover(2, *fib_public_program(true), transition=True)
    rng = np.random.default_rng(21)
    seen = set()
    for trial in range(24):
        t = t0.copy()
        if trial:
            t[int(rng.integers(0, 2)), int(rng.integers(0, 1 << h))] = int(rng.integers(0, 1 << 20))
        d = to_dev(torch, t)
        got = pr.check_constraints(d.data_ptr(), h)
        assert got == twin.check_constraints(d.data_ptr(), h), trial
        seen.add(got[0] > 0)
    assert seen == {False, True}
    # a wrong pv2 at proving time: the mock prover names the last row and that constraint, and the proof made is rejected
    wrong = true.copy()
    wrong[2] = (int(wrong[2]) + 1) % P
    pr.set_public_values(wrong)
    d = to_dev(torch, t0)
    assert pr.check_constraints(d.data_ptr(), h) == (1, (1 << h) - 1, 2)
    pf = prove(prover, [(pr, d, h)], False)
    assert (pf[9:12] == wrong).all()
    assert prover.verify_segment([(2, h, *cons, None)], pf, 6, 0, False, public=[3])[0] == (1 << 8) | 2
    assert prover.verify_segment([(2, h, *cons, None)], pf, 6, 0, False, public=[true])[0] == 17
    pr.close()
    twin.close()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    from powdr_amd import abi

    torch, prover = gpu
    h = 4
    t = fib_trace(h, 3, 5)
    d = to_dev(torch, t)
    pr = prover.Prover(2, *fib_public_program(), num_queries=4, n_public=3)
    assert prover.lib.pw_prover_n_public(pr._h) == 3
    # values never set: no proof, no mock proof — never with zeros in their place
    with pytest.raises(abi.HipError, match="hipError -1$"):
        prove(prover, [(pr, d, h)], False)
    with pytest.raises(abi.HipError):
        pr.check_constraints(d.data_ptr(), h)
    for bad in ([1, 2], [1, 2, 3, 4], [1, 2, P], [0xffffffff, 0, 0]):
        assert prover.lib.pw_prover_set_public_values(pr._h, prover._vp(np.array(bad, np.uint32)), len(bad)) == -1
        with pytest.raises(ValueError):
            pr.set_public_values(bad)
    with pytest.raises(abi.HipError):  # (a refused set leaves the values unset)
        prove(prover, [(pr, d, h)], False)
    pr.set_public_values(fib_public(t))
    assert prove(prover, [(pr, d, h)], False)[0] == MAGIC6
    # a segment proof only
    for call in (lambda: pr.prove(d.data_ptr(), h), lambda: pr.prove(d.data_ptr(), h, consume=True), lambda: pr.trace_root(d.data_ptr(), h),
                 lambda: prover.prove_airs([(pr, d.data_ptr(), h)])):
        with pytest.raises(abi.HipError, match="hipError -1$"):
            call()
    pr.close()
    # the entry itself: an operand behind the public values, too many of them, a degree above 3
    from powdr_amd.prover import row_operands

    r = row_operands(2)
    for cons, n in (([[PA, r.public(3)]], 3), ([[PA, r.public(0)]], 257), ([[PA, r.public(0), PA, 0, MUL, PA, 0, MUL, PA, 0, MUL, PA, 0, MUL]], 1)):
        with pytest.raises(RuntimeError):
            prover.Prover(2, *cons_tables(cons), n_public=n)


# ---- 7. three chained segments of one execution -----------------------------------------------------------------------------------------
CUTS = (0, 5, 9, 12)


@pytest.fixture(scope="module")
def chain(gpu):
    """one execution of 12 calls cut at call boundaries into segments of 5, 4 and 3 calls (its records sliced), each closed with the
    public connector and proven -> (execution, [Closed], [dict(descs, proof, public, preprocessed, logup, check_balance)])"""
    from powdr_amd import system_airs as sa
    from tests import test_system_airs_gpu as tsa

    torch, prover = gpu
    ex = vm.Execution(CUTS[-1], seed=5)
    mp = pytest.MonkeyPatch()
    mp.setattr(sa, "close_segment", functools.partial(sa.close_segment, public_connector=True))
    closed, segments = [], []
    try:
        for lo, hi in zip(CUTS, CUTS[1:]):
            piece = copy.copy(ex)
            piece.rec, piece.calls = np.ascontiguousarray(ex.rec[:, lo:hi]), hi - lo
            closed.append(tsa.Closed(gpu, piece))
    finally:
        mp.undo()
    for c in closed:
        segments.append(dict(descs=[(a["width"], a["log_h"], a["cons"][0], a["cons"][1], a["inter"]) for a in c.airs],
                             proof=prover.prove_segment(c.seg, logup=True),
                             public=[a.get("public") for a in c.airs],
                             preprocessed=[None if a["pre"] is None else (a["pre"][1], a["prover"].preprocessed_root()) for a in c.airs],
                             logup=True, check_balance=True))
    yield ex, closed, segments
    for c in closed:
        c.close()


def test_chained_segments(gpu, chain):
    from powdr_amd import system_airs as sa
    from tests import test_system_airs_gpu as tsa

    torch, prover = gpu
    ex, closed, segments = chain
    ci = [a["name"] for a in closed[0].airs].index("connector")
    states = []
    for c, g in zip(closed, segments):
        assert [a["name"] for a in c.airs].index("connector") == ci and g["proof"][0] == MAGIC6
        for a in c.airs:
            assert a["prover"].check_constraints(a["trace"].data_ptr(), a["log_h"]) == (0, None, None), a["name"]
        rc, total = prover.verify_segment(g["descs"], g["proof"], tsa.NQ, 0, True, check_balance=True, preprocessed=g["preprocessed"], public=g["public"])
        assert rc == 0 and not np.asarray(total).any()  # all six buses closed
        states.append(prover.segment_public_values(g["descs"], g["proof"], [None if v is None else len(v) for v in g["public"]], ci).tolist())
    # where the execution started and ended is what the first and the last proof say
    assert tuple(states[0][:2]) == ex.start and tuple(states[-1][2:]) == ex.end
    assert all(a[2:] == b[:2] for a, b in zip(states, states[1:])) and len({tuple(s) for s in states}) == 3
    links = sa.connector_links(ci)
    assert prover.verify_segment_chain(segments, links, tsa.NQ, 0) == (0, 0)
    # segments 2 and 3 swapped: segment 1 ends where segment 3 does not start — the first link from segment 0
    swapped = [segments[0], segments[2], segments[1]]
    assert prover.verify_segment_chain(swapped, links, tsa.NQ, 0) == (18, 0 * len(links) + 1)  # (the pc is the same everywhere: the timestamp link)
    # one query word of the second proof flipped: that segment's code and index
    bad = dict(segments[1])
    bad["proof"] = segments[1]["proof"].copy()
    bad["proof"][-3] ^= 1
    want = prover.verify_segment(bad["descs"], bad["proof"], tsa.NQ, 0, True, check_balance=True, preprocessed=bad["preprocessed"], public=bad["public"])[0]
    assert want not in (0, 1, 15, 17)
    assert prover.verify_segment_chain([segments[0], bad, segments[2]], links, tsa.NQ, 0) == (want, 1)
    # a link that names a value no AIR has
    assert prover.verify_segment_chain(segments, [(ci, 4, ci, 0)], tsa.NQ, 0)[0] == 18


def test_default_connector_keeps_todays_words(gpu, chain):
    """a segment closed with the default connector: no public values, the PWS5 words of a segment proof as it was"""
    from tests import test_system_airs_gpu as tsa

    torch, prover = gpu
    ex = chain[0]
    piece = copy.copy(ex)
    piece.rec, piece.calls = np.ascontiguousarray(ex.rec[:, :CUTS[1]]), CUTS[1]
    c = tsa.Closed(gpu, piece)
    assert all("public" not in a for a in c.airs) and c.by_name("connector")["air"].n_public == 0
    pf = prover.prove_segment(c.seg, logup=True)
    descs = [(a["width"], a["log_h"], a["cons"][0], a["cons"][1], a["inter"]) for a in c.airs]
    keys = [None if a["pre"] is None else (a["pre"][1], a["prover"].preprocessed_root()) for a in c.airs]
    assert pf[0] == MAGIC5
    rc, total = prover.verify_segment(descs, pf, tsa.NQ, 0, True, check_balance=True, preprocessed=keys, transition=True)
    assert rc == 0 and not np.asarray(total).any()
    # the same statement with the public connector differs from it only by the connector: header, values, the four constraints
    pub = chain[2][0]
    assert len(pub["proof"]) > len(pf) and pub["proof"][0] == MAGIC6
    c.close()
