"""The Poseidon2 compression chip on the device (pw_poseidon2_compress_trace, powdr_amd/system_airs.py poseidon2_air):
the generated trace against the numpy reference of tests/_poseidon2_air_ref.py word for word, the status codes, the constraint mock
prover on the device trace, a closed segment (hash users, the chip, the periphery AIRs) checked, proven and verified on both
expression paths, a wrong sender digest named by the bus check, a second round-constant table, and close_segment(poseidon2=True).
Every comparison is exact. The sizes are the smallest at which each path is taken: less than a wave, two AIRs of different heights
with more than one workgroup, and 2^16 keys from a first table of 64 slots (seven tables)."""
import ctypes as C

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _chained_vm as vm
from tests import _poseidon2_air_ref as ref
from tests.test_bus_check_gpu import BOTH_PATHS, NO_CONS, Segment, check_paths, from_dev, set_path, to_dev

pytestmark = pytest.mark.gpu
P = om.P
NQ = 4
BUS = 5
W = ref.WIDTH


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


def device_trace(seg, want, **kw):
    """the generated trace of the senders `seg`, compared with the reference trace `want` [307, rows]"""
    from powdr_amd import system_airs as sa

    cap = (want.shape[1] - 1).bit_length()
    trace, lh, rows, status = sa.poseidon2_compress_trace(seg, cap, **kw)
    assert status == 0 and 1 << lh == want.shape[1]
    got = from_dev(trace).reshape(W, 1 << lh)
    assert (got == want).all(), np.argwhere(got != want)[:5]
    return trace, rows


def assert_padding(want, n):
    zero = ref.permute(np.zeros((1, 16), np.int64), constants())[1][:, 0]
    assert zero[0] == 0 and (want[:, n:] == zero[:, None]).all() and want.shape[1] > n


@BOTH_PATHS
def test_three_requests_less_than_a_wave(gpu, monkeypatch, interpret):
    torch, prover = gpu
    set_path(monkeypatch, interpret)
    inputs = np.random.default_rng(1).integers(0, P, (3, 16), dtype=np.int64)
    host = [(ref.hash_user_trace(inputs, constants(), 2), ref.hash_user_interactions(BUS))]
    want, n = ref.compress_rows(ref.requests_of(host, BUS), constants())
    assert n == 3 and want.shape == (W, 4)
    assert_padding(want, 3)
    s = Segment(gpu, host)
    check_paths(s.provers, interpret)
    a, rows = device_trace(s.seg, want)
    b, _ = device_trace(s.seg, want)
    assert rows == 3 and torch.equal(a, b)
    s.close()


def two_senders():
    """2^10 requests: sender A (2^9 rows, all active) asks for 512 distinct keys once each; sender B (2^10 rows, two interactions on
    the same 24 words with multiplicities in columns 0 and 25) asks on 509 rows for keys A asked for — half of all requests are
    duplicates — sends one fresh key +1 on one row and -1 on another (its row keeps mult 0), and one fresh key 2 + 3 = 5 times from one
    row's two interactions"""
    rng = np.random.default_rng(2)
    k = constants()
    keys = rng.integers(0, P, (514, 16), dtype=np.int64)
    a = ref.hash_user_trace(keys[:512], k, 9)
    pick = rng.integers(0, 512, 512)
    pick[100], pick[300], pick[700 - 512 + 100] = 512, 512, 513
    b25 = ref.hash_user_trace(keys[pick], k, 10)
    rows = rng.permutation(1 << 10)[:512]  # the active rows of B, scattered over its four workgroups
    b = np.zeros((26, 1 << 10), np.uint32)
    b[:25, rows] = b25[:, :512]
    b[0, rows[300]] = P - 1
    b[0, rows[288]], b[25, rows[288]] = 2, 3
    words = [[0, c] for c in range(1, 25)]
    spans, bc = [], []
    for prog in [[0, 0]] + words + [[0, 25]] + words:
        spans.append((len(bc), 2))
        bc += prog
    it_b = (np.array([[BUS, 24, 0], [BUS, 24, 25]], np.uint32), np.array(spans, np.uint32), np.array(bc, np.uint32))
    return [(a, ref.hash_user_interactions(BUS)), (b, it_b)], keys, rows


@BOTH_PATHS
def test_two_senders_with_duplicates_a_cancelled_key_and_five_from_one_row(gpu, monkeypatch, interpret):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    set_path(monkeypatch, interpret)
    host, keys, rows = two_senders()
    requests = ref.requests_of(host, BUS)
    assert len(requests) == (1 << 10) + 1  # (the row with two interactions counts twice)
    want, n = ref.compress_rows(requests, constants())
    assert n == 514 and want.shape == (W, 1 << 10)
    assert_padding(want, n)
    by_key = {tuple(want[1:17, r].tolist()): int(want[0, r]) for r in range(n)}
    assert by_key[tuple(keys[512].tolist())] == 0 and by_key[tuple(keys[513].tolist())] == 5 and sum(by_key.values()) == 512 + 509 + 0 + 5
    s = Segment(gpu, host)
    check_paths(s.provers, interpret)
    a, got_rows = device_trace(s.seg, want)
    assert got_rows == 514
    st = sa.last_stats()
    assert st["occupied_slots"] == 514 and st["tables"] == 1 and st["walked"] == (1 << 9) + 2 * (1 << 10) and st["scratch_bytes"] < 64 << 10 < st["peak_bytes"]
    b, _ = device_trace(s.seg, want, start_log_slots=6)
    assert torch.equal(a, b) and sa.last_stats()["tables"] >= 3  # another table, another order of arrival: the same bytes
    # the chip's trace closes the bus (the senders' digests are right) and satisfies the constraints
    air = sa.poseidon2_air()
    p = air.make_prover(NQ)
    assert p.max_constraint_degree() == 3 and p.check_constraints(a.data_ptr(), 10) == (0, None, None)
    summaries, tuples = prover.check_segment_buses(s.seg + [(p, a.data_ptr(), 10)], buses=[BUS], tally_all=True)
    assert summaries == [dict(bus=BUS, status=0, n_active=1025 + 513, n_unbalanced=0)] and tuples == []
    p.close()
    s.close()


def test_two_to_the_16_keys_from_a_table_of_64_slots(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    n = 1 << 16
    inputs = np.random.default_rng(3).integers(0, P, (n, 16), dtype=np.int64)
    user = np.zeros((ref.USER_WIDTH, n), np.uint32)  # (the digests are not read: left zero)
    user[0], user[1:17] = 1, inputs.T
    host = [(user, ref.hash_user_interactions(BUS))]
    want = ref.permute(inputs, constants())[1].astype(np.uint32)
    want[0] = 1
    s = Segment(gpu, host)
    a, rows = device_trace(s.seg, want, start_log_slots=6)
    st = sa.last_stats()
    assert rows == n and st["tables"] >= 3 and st["occupied_slots"] == n and st["table_slots"] == 1 << 17  # (never more than twice the triples walked)
    b, _ = device_trace(s.seg, want, start_log_slots=6)
    c, _ = device_trace(s.seg, want)
    assert torch.equal(a, b) and torch.equal(a, c) and sa.last_stats()["tables"] == 2
    # a bound of one table of 2^16 slots holds 7/8 of them: status 2, every time, nothing written
    out = torch.full((W << 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for _ in range(2):
        assert sa.poseidon2_compress_trace(s.seg, 16, table_bytes=32 << 16, out=out) == (None, 0, 0, 2)
    assert sa.poseidon2_compress_trace(s.seg, 16, table_bytes=31, out=out)[3] == 2
    assert bool((out == 0x5A5A5A5A).all())
    s.close()


def test_status_codes_and_refusals(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import abi
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    inputs = np.random.default_rng(4).integers(0, P, (100, 16), dtype=np.int64)
    host = [(ref.hash_user_trace(inputs, constants(), 7), ref.hash_user_interactions(BUS))]
    want, _ = ref.compress_rows(ref.requests_of(host, BUS), constants())
    s = Segment(gpu, host)
    # 1: the cap is too small: what is needed comes back, the caller's buffer is untouched; without a buffer the call retries
    out = torch.full((W << 7,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert sa.poseidon2_compress_trace(s.seg, 3, out=out) == (None, 7, 100, 1)
    assert bool((out == 0x5A5A5A5A).all())
    trace, lh, rows, status = sa.poseidon2_compress_trace(s.seg, 3)
    assert (lh, rows, status) == (7, 100, 0) and (from_dev(trace).reshape(W, -1) == want).all()
    trace, lh, rows, status = sa.poseidon2_compress_trace(s.seg, 7, out=out)
    assert status == 0 and trace.data_ptr() == out.data_ptr() and (from_dev(trace).reshape(W, -1) == want).all()
    # -1: an interaction on the bus with 23 arguments; a NULL output; a cap of 0; a first table outside 2^6 .. 2^30
    s23 = Segment(gpu, host + [(host[0][0][:24], ref.hash_user_interactions(BUS, 23))])
    with pytest.raises(abi.HipError):
        sa.poseidon2_compress_trace(s23.seg, 8)
    recs, n = sa._records(s.seg)
    lh_, rows_, status_ = C.c_uint32(), C.c_uint64(), C.c_uint32()
    assert sa.lib.pw_poseidon2_compress_trace(recs, n, BUS, 0, 0, None, 7, C.byref(lh_), C.byref(rows_), C.byref(status_)) == -1
    assert sa.lib.pw_poseidon2_compress_trace(recs, n, BUS, 0, 0, out.data_ptr(), 7, None, C.byref(rows_), C.byref(status_)) == -1
    for kw in (dict(cap_log_height=0), dict(cap_log_height=7, start_log_slots=5), dict(cap_log_height=7, start_log_slots=31)):
        with pytest.raises(abi.HipError):
            sa.poseidon2_compress_trace(s.seg, out=out, **kw)
    # a bus nobody sends on: two padding rows
    trace, lh, rows, status = sa.poseidon2_compress_trace(s.seg, 1, bus=77)
    assert (lh, rows, status) == (1, 0, 0) and (from_dev(trace).reshape(W, 2) == ref.compress_rows([], constants())[0]).all()
    s.close()
    s23.close()


# ---- the closed segment: hash users, the chip, the periphery AIRs -------------------------------------------------------------------
class HashSegment:
    """two hash users at 2^10 and 2^8 rows — the second also range-checks left[0] (below 2^17) — the chip made from what they send,
    and the three periphery AIRs in the preprocessed layout"""

    def __init__(self, gpu, tamper=None):
        torch, prover = gpu
        from powdr_amd import periphery, tracegen
        from powdr_amd import system_airs as sa
        from powdr_amd.segment_workload import BusReplay

        rng = np.random.default_rng(6)
        k = constants()
        in_a = rng.integers(0, P, (1000, 16), dtype=np.int64)
        in_a[:200, 0] %= 1 << 17
        in_b = np.concatenate([rng.integers(0, P, (24, 16), dtype=np.int64), in_a[:200]])  # 200 of its 224 requests repeat user 0's
        in_b[:, 0] %= 1 << 17
        users = [(ref.hash_user_trace(in_a, k, 10), ref.hash_user_interactions(BUS)),
                 (ref.hash_user_trace(in_b, k, 8), ref.hash_user_interactions(BUS, range_bus=3))]
        if tamper is not None:
            tamper(users)
        self.host = users
        self.per = tracegen.Periphery.fresh()
        self.airs = []
        for i, (t, it) in enumerate(users):
            lh = t.shape[1].bit_length() - 1
            p = prover.Prover(t.shape[0], *NO_CONS, num_queries=NQ, interactions=it)
            self.airs.append(dict(name=f"user{i}", role="user", width=t.shape[0], log_h=lh, cons=NO_CONS, inter=it, trace=to_dev(torch, t), prover=p, pre=None))
        torch.cuda.synchronize()
        self.senders = [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in self.airs]
        for a in self.airs:
            BusReplay(a["inter"], 1 << a["log_h"])(a["trace"].data_ptr(), self.per)
        self.air = sa.poseidon2_air()
        trace, lh, self.rows, status = sa.poseidon2_compress_trace(self.senders, 4)
        assert status == 0
        self.airs.append(dict(name="poseidon2", role="system", width=W, log_h=lh, cons=self.air.cons, inter=self.air.inter, trace=trace,
                              prover=self.air.make_prover(NQ), pre=None))
        per = self.per
        for name, hist, it, table, pre_w in (("var_range", per.var_hist, periphery.var_range_interactions_pre(), periphery.var_range_table(per.var_hist.numel()), 2),
                                             ("tuple2", per.tuple_hist, periphery.tuple2_interactions_pre(), periphery.tuple2_table(per.tuple_sizes), 2),
                                             ("bitwise", per.bitwise_hist, periphery.bitwise_interactions_pre(), periphery.bitwise_table(), 3)):
            lh = (hist.numel() // (2 if name == "bitwise" else 1)).bit_length() - 1
            torch.cuda.synchronize()
            pre = (table, pre_w, lh)
            p = prover.Prover(hist.numel() >> lh, *NO_CONS, num_queries=NQ, interactions=it, preprocessed=pre)
            self.airs.append(dict(name=name, role="periphery", width=hist.numel() >> lh, log_h=lh, cons=NO_CONS, inter=it, trace=periphery.multiplicities(hist),
                                  prover=p, pre=pre))
        torch.cuda.synchronize()

    @property
    def seg(self):
        return [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in self.airs]

    def descs(self):
        return [(a["width"], a["log_h"], a["cons"][0], a["cons"][1], a["inter"]) for a in self.airs]

    def keys(self):
        return [None if a["pre"] is None else (a["pre"][1], a["prover"].preprocessed_root()) for a in self.airs]

    def close(self):
        for a in self.airs:
            a["prover"].close()


def test_the_closed_segment_is_checked_proven_and_verified_on_both_paths(gpu, monkeypatch):
    torch, prover = gpu
    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    h = HashSegment(gpu)
    want, n = ref.compress_rows(ref.requests_of(h.host, BUS), constants())
    chip = h.airs[2]
    assert n == h.rows == 1024 and chip["log_h"] == 10 and (from_dev(chip["trace"]).reshape(W, -1) == want).all()
    summaries, tuples = prover.check_segment_buses(h.seg)
    assert [(s["bus"], s["status"]) for s in summaries] == [(3, 0), (BUS, 0), (6, 0), (7, 0)] and tuples == []
    assert summaries[1]["n_active"] == 1224 + 1024 and summaries[0]["n_active"] > 224
    proofs = {}
    for jit in ("0", "1"):
        monkeypatch.setenv("POWDR_JIT", jit)
        p = h.air.make_prover(NQ)
        assert p.max_constraint_degree() == 3 and p.check_constraints(chip["trace"].data_ptr(), 10) == (0, None, None)
        seg = [(p, t, lh) if a["name"] == "poseidon2" else (q, t, lh) for a, (q, t, lh) in zip(h.airs, h.seg)]
        proofs[jit] = prover.prove_segment(seg, logup=True)
        assert p.specialised()["state"] == (1 if jit == "1" else 0)
        rc, total = prover.verify_segment(h.descs(), proofs[jit], NQ, 0, True, check_balance=True, preprocessed=h.keys())
        assert rc == 0 and not np.asarray(total).any()
        p.close()
    assert len(proofs["0"]) == len(proofs["1"]) and (proofs["0"] == proofs["1"]).all()
    # one cell of the chip's trace off by one: the mock prover and the verifier refuse it
    bad = chip["trace"].clone()
    bad[(ref.PARTIAL + 7) * 1024 + 33] += 1
    n_bad, row, _ = chip["prover"].check_constraints(bad.data_ptr(), 10)
    assert n_bad >= 1 and row == 33
    h.close()


def test_one_wrong_sender_digest_is_named_by_the_bus_check(gpu, monkeypatch):
    torch, prover = gpu
    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ROW = 321
    honest = {}

    def tamper(users):
        t = users[0][0]
        honest.update(args=t[1:25, ROW].tolist())
        t[17 + 5, ROW] = (int(t[17 + 5, ROW]) + 1) % P

    h = HashSegment(gpu, tamper)
    chip = h.airs[2]
    want, n = ref.compress_rows(ref.requests_of(h.host, BUS), constants())
    assert (from_dev(chip["trace"]).reshape(W, -1) == want).all()  # still written, and the same trace: the digests are not read
    assert chip["prover"].check_constraints(chip["trace"].data_ptr(), 10) == (0, None, None)
    summaries, tuples = prover.check_segment_buses(h.seg, buses=[BUS])
    assert summaries == [dict(bus=BUS, status=1, n_active=1224 + 1024, n_unbalanced=2)] and len(tuples) == 2
    sent = next(t for t in tuples if t["net_multiplicity"] == 1)
    lost = next(t for t in tuples if t["net_multiplicity"] == P - 1)
    assert (sent["air"], sent["interaction"], sent["row"], sent["n_args"]) == (0, 0, ROW, 24)
    assert sent["args"] == honest["args"][:16] == lost["args"] and lost["air"] == 2
    assert from_dev(chip["trace"]).reshape(W, -1)[1:17, lost["row"]].tolist() == honest["args"][:16]
    h.close()


def test_a_second_constant_table(gpu, monkeypatch):
    torch, prover = gpu
    from oracle import stark_model as sm
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    first = sa.poseidon2_air()
    rng = np.random.default_rng(0xC0FFEE)
    E, I = rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32)
    prover.set_poseidon2_constants(E, I)
    sm.set_poseidon2_constants(E, I)
    try:
        h = HashSegment(gpu)
        chip = h.airs[2]
        want, n = ref.compress_rows(ref.requests_of(h.host, BUS), constants())
        assert (constants()[0] == E).all() and (from_dev(chip["trace"]).reshape(W, -1) == want).all()
        assert chip["prover"].check_constraints(chip["trace"].data_ptr(), 10) == (0, None, None)
        stale = first.make_prover(NQ)  # the AIR of the other table does not hold on these rows
        assert stale.check_constraints(chip["trace"].data_ptr(), 10)[0] > 0
        stale.close()
        proof = prover.prove_segment(h.seg, logup=True)
        rc, total = prover.verify_segment(h.descs(), proof, NQ, 0, True, check_balance=True, preprocessed=h.keys())
        assert rc == 0 and not np.asarray(total).any()
        h.close()
    finally:
        prover.set_poseidon2_constants()
        sm.set_poseidon2_constants()


# ---- close_segment(..., poseidon2=True) -----------------------------------------------------------------------------------------------
def closed_execution(gpu, ex, with_user, **kw):
    """tests/test_system_airs_gpu.py Closed with one hash user among the senders and close_segment's keywords passed on"""
    torch, prover = gpu
    from powdr_amd import periphery, tracegen
    from powdr_amd import system_airs as sa
    from powdr_amd.segment_workload import BusReplay

    per = tracegen.Periphery.fresh()
    airs = []
    for name, t, (bc, sp, it) in ex.instruction_airs():
        lh = t.shape[1].bit_length() - 1
        p = prover.Prover(t.shape[0], bc, sp, num_queries=NQ, interactions=it)
        airs.append(dict(name=name, role="instruction", width=t.shape[0], log_h=lh, cons=(bc, sp), inter=it, trace=to_dev(torch, t), prover=p, pre=None))
    if with_user:
        inputs = np.random.default_rng(9).integers(0, P, (40, 16), dtype=np.int64)
        t, it = ref.hash_user_trace(inputs, constants(), 6), ref.hash_user_interactions(BUS)
        airs.append(dict(name="user", role="user", width=t.shape[0], log_h=6, cons=NO_CONS, inter=it, trace=to_dev(torch, t),
                         prover=prover.Prover(t.shape[0], *NO_CONS, num_queries=NQ, interactions=it), pre=None))
    torch.cuda.synchronize()
    for a in airs:
        BusReplay(a["inter"], 1 << a["log_h"])(a["trace"].data_ptr(), per)
    airs = sa.close_segment(airs, ex.program_table(), ex.start_pc, per, num_queries=NQ, **kw)
    for name, hist, it, table, pre_w in (("var_range", per.var_hist, periphery.var_range_interactions_pre(), periphery.var_range_table(per.var_hist.numel()), 2),
                                         ("tuple2", per.tuple_hist, periphery.tuple2_interactions_pre(), periphery.tuple2_table(per.tuple_sizes), 2),
                                         ("bitwise", per.bitwise_hist, periphery.bitwise_interactions_pre(), periphery.bitwise_table(), 3)):
        lh = (hist.numel() // (2 if name == "bitwise" else 1)).bit_length() - 1
        torch.cuda.synchronize()
        pre = (table, pre_w, lh)
        p = prover.Prover(hist.numel() >> lh, *NO_CONS, num_queries=NQ, interactions=it, preprocessed=pre)
        airs.append(dict(name=name, role="periphery", width=hist.numel() >> lh, log_h=lh, cons=NO_CONS, inter=it, trace=periphery.multiplicities(hist), prover=p, pre=pre))
    torch.cuda.synchronize()
    return airs


def test_close_segment_appends_the_chip_when_asked_and_changes_nothing_otherwise(gpu, monkeypatch):
    torch, prover = gpu
    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex = vm.Execution(64, seed=7)
    seg_of = lambda airs: [(a["prover"], a["trace"].data_ptr(), a["log_h"]) for a in airs]
    closed = closed_execution(gpu, ex, True, poseidon2=True)
    names = [a["name"] for a in closed]
    assert names[names.index("program"):names.index("program") + 4] == ["program", "connector", "boundary", "poseidon2"]
    chip = closed[names.index("poseidon2")]
    assert chip["log_h"] == 6 and chip["width"] == W
    summaries, tuples = prover.check_segment_buses(seg_of(closed))
    assert [s["bus"] for s in summaries] == [0, 1, 2, 3, BUS, 6, 7] and all(s["status"] == 0 and s["n_active"] > 0 for s in summaries) and tuples == []
    # the same senders without the flag: the compression bus stays open
    left_open = closed_execution(gpu, ex, True)
    assert "poseidon2" not in [a["name"] for a in left_open]
    assert [(s["bus"], s["status"]) for s in prover.check_segment_buses(seg_of(left_open), tuple_cap=4)[0]] == [(0, 0), (1, 0), (2, 0), (3, 0), (BUS, 1), (6, 0), (7, 0)]
    # without a hash user the flag appends nothing, and False is the call without the keyword: the same proof words
    proofs = []
    for kw in (dict(), dict(poseidon2=False), dict(poseidon2=True)):
        airs = closed_execution(gpu, ex, False, **kw)
        assert [a["name"] for a in airs][-6:] == ["program", "connector", "boundary", "var_range", "tuple2", "bitwise"]
        proofs.append(prover.prove_segment(seg_of(airs), logup=True))
        for a in airs:
            a["prover"].close()
    assert all(len(p) == len(proofs[0]) and (p == proofs[0]).all() for p in proofs[1:])
    for a in closed + left_open:
        a["prover"].close()
