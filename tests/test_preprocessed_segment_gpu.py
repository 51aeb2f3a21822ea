"""pw-stark v1 + preprocessed columns on the device: the preprocessed commitment is the oracle's one-AIR main
commitment of the fixed matrix, the periphery tables split into fixed part and multiplicities, constraints and interactions read fixed
columns on every expression path, the forged range check that the main-column layout accepts is rejected, tampering with the
preprocessed openings is caught, and the C4 workload in the preprocessed layout proves, verifies and balances."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm

pytestmark = pytest.mark.gpu
P = om.P
PA, PC, ADD, SUB, MUL, NEG = 0, 1, 2, 3, 4, 5
MAGIC3, MAGIC4 = 0x33535750, 0x34535750
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))
NO_INTER = (np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32))


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import periphery, prover

    return torch, prover, periphery


def to_dev(torch, canonical):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(canonical, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()


def from_dev(t):
    return om.from_monty(t.cpu().numpy().view(np.uint32))


def tables(rows):
    """rows: [(bus, mult program, [arg programs])] -> (interactions, spans, bytecode)"""
    inter, spans, bc = [], [], []
    for bus, m, args in rows:
        inter.append((bus, len(args), len(spans)))
        for prog in [m] + args:
            spans.append((len(bc), len(prog)))
            bc += prog
    return np.array(inter, np.uint32).reshape(-1, 3), np.array(spans, np.uint32).reshape(-1, 2), np.array(bc, np.uint32)


def cons_tables(progs):
    bc, spans = [], []
    for p in progs:
        spans.append((len(bc), len(p)))
        bc += p
    return np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)


# ---- 1. the key ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [1, 4, 10, 14])
def test_preprocessed_root_is_the_oracle_main_commitment_of_the_fixed_matrix(gpu, h):
    torch, prover, _ = gpu
    rng = np.random.default_rng(h)
    Wf = 3
    fixed = rng.integers(0, P, (Wf, 1 << h), dtype=np.uint64).astype(np.uint32)
    pr = prover.Prover(1, *NO_CONS, num_queries=4, preprocessed=(to_dev(torch, fixed), Wf, h))
    want = sm.prove_segment([(fixed.reshape(-1), Wf, h, *NO_CONS, None)], num_queries=0, logup=False)[9:17]
    assert (pr.preprocessed_root() == want).all()
    assert pr.device_bytes() >= Wf * (3 << h) * 4  # the fixed matrix, its LDE (and its tree) are the prover's
    # a one-AIR v0 proof, a trace root or independent proofs of such a prover: -1 (segment proofs only)
    t = to_dev(torch, np.zeros(1 << h, np.uint32))
    for call in (lambda: pr.prove(t.data_ptr(), h), lambda: pr.trace_root(t.data_ptr(), h), lambda: prover.prove_airs([(pr, t.data_ptr(), h)])):
        with pytest.raises(RuntimeError):
            call()
    pr.close()


def test_malformed_preprocessed_programs_get_no_prover(gpu):
    torch, prover, _ = gpu
    fixed = to_dev(torch, np.zeros(2 * 16, np.uint32))
    ok = cons_tables([[PA, 0, PA, 2, MUL]])  # column 2 = preprocessed column 0 of a width-1 AIR with 2 fixed columns
    prover.Prover(1, *ok, preprocessed=(fixed, 2, 4)).close()
    with pytest.raises(RuntimeError):
        prover.Prover(1, *cons_tables([[PA, 3]]), preprocessed=(fixed, 2, 4))  # 3 >= W + Wp
    with pytest.raises(RuntimeError):
        prover.Prover(1, *NO_CONS, interactions=tables([(3, [PA, 0], [[PA, 3]])]), preprocessed=(fixed, 2, 4))


# ---- 2. the periphery kernels ---------------------------------------------------------------------------------------------------
def test_periphery_tables_and_multiplicities(gpu):
    torch, _, periphery = gpu
    rng = np.random.default_rng(2)
    for bins in (1, 16, 1 << 18):
        assert (from_dev(periphery.var_range_table(bins)).reshape(2, bins) == om.var_range_trace(np.zeros(bins, np.uint32))[:2]).all()
        h = rng.integers(0, 1 << 32, bins, dtype=np.uint64).astype(np.uint32)
        h[0] = P  # counts >= p are reduced
        got = from_dev(periphery.multiplicities(torch.from_numpy(h.view(np.int32)).cuda()))
        assert (got == om.var_range_trace(h)[2]).all()
    for sz in ((256, 2048), (4, 8)):
        n = sz[0] * sz[1]
        assert (from_dev(periphery.tuple2_table(sz)).reshape(2, n) == om.tuple2_trace(np.zeros(n, np.uint32), *sz)[:2]).all()
        h = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        assert (from_dev(periphery.multiplicities(torch.from_numpy(h.view(np.int32)).cuda())) == om.tuple2_trace(h, *sz)[2]).all()
    assert (from_dev(periphery.bitwise_table()).reshape(3, 65536) == om.bitwise_trace(np.zeros(2 * 65536, np.uint32))[:3]).all()
    h = rng.integers(0, 1 << 32, 2 * 65536, dtype=np.uint64).astype(np.uint32)
    h[7], h[65536 + 9] = P, P + 3
    got = from_dev(periphery.multiplicities(torch.from_numpy(h.view(np.int32)).cuda())).reshape(2, 65536)
    assert (got == om.bitwise_trace(h)[3:]).all()


# ---- 3. constraints and interactions over fixed columns ---------------------------------------------------------------------------
# main [a, b] | pre [sel, ramp] (operands 2, 3): sel = 1 on row 0, ramp = row index.  sel (a - 7) = 0, b - ramp a = 0; bus 9 sends
# (a, ramp) `sel` times.
RAMP_CONS = cons_tables([[PA, 2, PA, 0, PC, 7, SUB, MUL], [PA, 1, PA, 3, PA, 0, MUL, SUB]])
RAMP_INTER = tables([(9, [PA, 2], [[PA, 0], [PA, 3]])])
SQ_CONS = cons_tables([[PA, 1, PA, 0, PA, 0, MUL, SUB]])  # a plain AIR beside them: b = a^2


def ramp_fixed(h):
    H = 1 << h
    sel = np.zeros(H, np.uint32)
    sel[0] = 1
    return np.stack([sel, np.arange(H, dtype=np.uint32)])


def ramp_trace(h, seed):
    H = 1 << h
    a = np.random.default_rng(seed).integers(0, P, H, dtype=np.uint64)
    a[0] = 7
    return np.stack([a, a * np.arange(H, dtype=np.uint64) % P]).astype(np.uint32)


RAMP_HEIGHTS, SQ_HEIGHT = (5, 6, 8), 7


def ramp_segment(torch, prover, nq=5):
    """-> (provers, device traces, log heights, descriptions, keys) of 3 ramp AIRs + 1 plain AIR"""
    provers, traces, lhs, descs, keys = [], [], [], [], []
    for k, h in enumerate(RAMP_HEIGHTS):
        pr = prover.Prover(2, *RAMP_CONS, num_queries=nq, pow_bits=2, interactions=RAMP_INTER, preprocessed=(to_dev(torch, ramp_fixed(h)), 2, h))
        provers.append(pr)
        traces.append(to_dev(torch, ramp_trace(h, k)))
        lhs.append(h)
        descs.append((2, h, *RAMP_CONS, RAMP_INTER))
        keys.append((2, pr.preprocessed_root()))
    a = np.random.default_rng(9).integers(0, P, 1 << SQ_HEIGHT, dtype=np.uint64)
    provers.append(prover.Prover(2, *SQ_CONS, num_queries=nq, pow_bits=2, interactions=NO_INTER))
    traces.append(to_dev(torch, np.stack([a, a * a % P]).astype(np.uint32)))
    lhs.append(SQ_HEIGHT)
    descs.append((2, SQ_HEIGHT, *SQ_CONS, NO_INTER))
    keys.append(None)
    return provers, traces, lhs, descs, keys


def prove(prover, provers, traces, lhs):
    return prover.prove_segment([(p, t.data_ptr(), h) for p, t, h in zip(provers, traces, lhs)], logup=True)


def test_constraints_over_fixed_columns_on_every_path(gpu, monkeypatch):
    torch, prover, _ = gpu
    provers, traces, lhs, descs, keys = ramp_segment(torch, prover)
    for p, t, h in zip(provers, traces, lhs):
        assert p.check_constraints(t.data_ptr(), h)[0] == 0
    pf = prove(prover, provers, traces, lhs)
    assert pf[0] == MAGIC4
    assert prover.verify_segment(descs, pf, 5, 2, True, preprocessed=keys)[0] == 0
    assert prover.verify_segment(descs, pf, 5, 2, True)[0] == 1  # the verifying key is part of the statement
    monkeypatch.setenv("POWDR_SEGMENT_STREAMS", "0")
    assert (prove(prover, provers, traces, lhs) == pf).all()
    monkeypatch.delenv("POWDR_SEGMENT_STREAMS")
    # a trace wrong only on the selected row: the mock prover names row 0, the proof does not verify
    bad = ramp_trace(lhs[1], 1)
    bad[0, 0] = 8
    bad_t = to_dev(torch, bad)
    n, row, c = provers[1].check_constraints(bad_t.data_ptr(), lhs[1])
    assert n == 1 and row == 0 and c == 0
    bad_traces = list(traces)
    bad_traces[1] = bad_t
    assert prover.verify_segment(descs, prove(prover, provers, bad_traces, lhs), 5, 2, True, preprocessed=keys)[0] != 0
    # the interpreter (above: small forms for the interactions), POWDR_LOGUP_INTERPRET=1, the specialised kernels: the same words
    monkeypatch.setenv("POWDR_LOGUP_INTERPRET", "1")
    interp = ramp_segment(torch, prover)[0]
    monkeypatch.delenv("POWDR_LOGUP_INTERPRET")
    assert [p.logup_path() for p in provers[:3]] == [2, 2, 2] and [p.logup_path() for p in interp[:3]] == [1, 1, 1]
    assert (prove(prover, interp, traces, lhs) == pf).all()
    prover.specialise_all(provers)
    assert [p.specialised()["state"] for p in provers[:3]] == [1, 1, 1]
    assert (prove(prover, provers, traces, lhs) == pf).all()
    with pytest.raises(RuntimeError):  # another height than the fixed matrix's
        prove(prover, provers, traces, [lhs[0] + 1] + lhs[1:])
    for p in provers + interp:
        p.close()


# ---- 4. the forgery that motivated this ---------------------------------------------------------------------------------------------
SEND = tables([(3, [PA, 2], [[PA, 0], [PA, 1]])])  # sender [v, bits, m]: sends (v, bits) m times
BINS_LOG = 9


def sender_trace(v, bits):
    t = np.zeros((3, 4), np.uint32)
    t[:, 0] = (v, bits, 1)
    return t


def test_a_forged_range_check_balances_in_the_main_layout_and_not_in_the_preprocessed_one(gpu):
    torch, prover, periphery = gpu
    nb = 1 << BINS_LOG
    snd = prover.Prover(3, *NO_CONS, num_queries=4, interactions=SEND)
    forged = to_dev(torch, sender_trace(300, 8))
    # today's layout: the receiver's tuple columns are committed, nothing constrains them — a forged row balances the send
    recv_t = om.var_range_trace(np.zeros(nb, np.uint32))
    recv_t[:, 0] = (300, 8, 1)
    rcv = prover.Prover(3, *NO_CONS, num_queries=4, interactions=periphery.var_range_interactions())
    recv_d = to_dev(torch, recv_t)
    pf = prover.prove_segment([(snd, forged.data_ptr(), 2), (rcv, recv_d.data_ptr(), BINS_LOG)], logup=True)
    descs = [(3, 2, *NO_CONS, SEND), (3, BINS_LOG, *NO_CONS, periphery.var_range_interactions())]
    rc, total = prover.verify_segment(descs, pf, 4, 0, True, check_balance=True)
    assert rc == 0 and not total.any()  # the hole
    # the chips' layout: the table is the key's, the prover chooses only multiplicities — no choice balances (300, 8)
    table = periphery.var_range_table(nb)
    pre = prover.Prover(1, *NO_CONS, num_queries=4, interactions=periphery.var_range_interactions_pre(), preprocessed=(table, 2, BINS_LOG))
    keys = [None, (2, pre.preprocessed_root())]
    descs = [(3, 2, *NO_CONS, SEND), (1, BINS_LOG, *NO_CONS, periphery.var_range_interactions_pre())]
    rng = np.random.default_rng(4)
    for mult in (np.zeros(nb, np.uint32), np.eye(1, nb, (1 << 8) + 44 - 1, dtype=np.uint32)[0], rng.integers(0, 3, nb).astype(np.uint32)):
        mult_t = to_dev(torch, mult)
        pf = prover.prove_segment([(snd, forged.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)], logup=True)
        assert prover.verify_segment(descs, pf, 4, 0, True, preprocessed=keys)[0] == 0  # a valid proof ...
        assert prover.verify_segment(descs, pf, 4, 0, True, check_balance=True, preprocessed=keys)[0] == 14  # ... of an unbalanced bus
    # an honest in-range send balances
    honest = to_dev(torch, sender_trace(200, 8))
    mult = np.zeros(nb, np.uint32)
    mult[(1 << 8) + 200 - 1] = 1
    mult_t = to_dev(torch, mult)
    pf = prover.prove_segment([(snd, honest.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)], logup=True)
    rc, total = prover.verify_segment(descs, pf, 4, 0, True, check_balance=True, preprocessed=keys)
    assert rc == 0 and not total.any()
    for p in (snd, rcv, pre):
        p.close()


# ---- 5. tampering ---------------------------------------------------------------------------------------------------------------------
def test_tampered_preprocessed_openings_and_keys_are_rejected(gpu):
    torch, prover, periphery = gpu
    nb, nq = 1 << BINS_LOG, 4
    snd = prover.Prover(3, *NO_CONS, num_queries=nq, interactions=SEND)
    table = periphery.var_range_table(nb)
    inter = periphery.var_range_interactions_pre()
    pre = prover.Prover(1, *NO_CONS, num_queries=nq, interactions=inter, preprocessed=(table, 2, BINS_LOG))
    mult = np.zeros(nb, np.uint32)
    mult[(1 << 8) + 200 - 1] = 1
    send_t, mult_t = to_dev(torch, sender_trace(200, 8)), to_dev(torch, mult)  # (alive while the segment is proven)
    pf = prover.prove_segment([(snd, send_t.data_ptr(), 2), (pre, mult_t.data_ptr(), BINS_LOG)], logup=True)
    descs = [(3, 2, *NO_CONS, SEND), (1, BINS_LOG, *NO_CONS, inter)]
    keys = [None, (2, pre.preprocessed_root())]
    assert prover.verify_segment(descs, pf, nq, 0, True, check_balance=True, preprocessed=keys)[0] == 0
    # word positions: header, main root, perm root, sums, quotient root, openings, FRI roots, final value, witness
    Wp = [4 * len(prover.logup_group_starts(SEND)), 4 * len(prover.logup_group_starts(inter))]
    K = [3 + 2 * Wp[0] + 8, 1 + 2 + 2 * Wp[1] + 8]
    L = BINS_LOG + 1
    opened = 5 + 4 * 2 + 8 + 8 + 4 * 2 + 8
    q0 = opened + 4 * sum(K) + 8 * (L - 1) + 4 + 1
    assert pf[q0] < (1 << L)
    pre_row = q0 + 1 + (3 + 1) + 8 * L  # after the main tree's answer
    for pos, want in ((pre_row, 16), (pre_row + 1, 16), (pre_row + 2, 16), (pre_row + 2 + 8 * L - 1, 16)):
        bad = pf.copy()
        bad[pos] = (int(bad[pos]) + 1) % P
        assert prover.verify_segment(descs, bad, nq, 0, True, preprocessed=keys)[0] == want, pos
    bad = pf.copy()
    bad[opened + 4 * (K[0] + 1)] = (int(bad[opened + 4 * (K[0] + 1)]) + 1) % P  # the receiver's first preprocessed value at zeta
    assert prover.verify_segment(descs, bad, nq, 0, True, preprocessed=keys)[0] != 0
    # a key with one table entry changed, a wrong preprocessed width
    other = from_dev(table).reshape(2, nb)
    other[0, 5] = (int(other[0, 5]) + 1) % P
    pre2 = prover.Prover(1, *NO_CONS, num_queries=nq, interactions=inter, preprocessed=(to_dev(torch, other), 2, BINS_LOG))
    assert not (pre2.preprocessed_root() == keys[1][1]).all()
    assert prover.verify_segment(descs, pf, nq, 0, True, preprocessed=[None, (2, pre2.preprocessed_root())])[0] != 0
    assert prover.verify_segment(descs, pf, nq, 0, True, preprocessed=[None, (3, keys[1][1])])[0] != 0
    assert prover.verify_segment(descs, pf, nq, 0, True, preprocessed=[None, (1, keys[1][1])])[0] != 0
    # an operand past the combined bound in a description: 15
    bad_inter = (inter[0], inter[1], inter[2].copy())
    bad_inter[2][bad_inter[2].tolist().index(2, 3)] = 3  # the `bits` operand (column 2) -> column 3 = W + Wp
    assert prover.verify_segment([descs[0], (1, BINS_LOG, *NO_CONS, bad_inter)], pf, nq, 0, True, preprocessed=keys)[0] == 15
    for p in (snd, pre, pre2):
        p.close()


# ---- 6 / 7. the workload ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workload(gpu):
    from powdr_amd import segment_workload as sw

    seg = sw.HonestSegment("C4", max_log_height=9, seed=2, queries=4, pow_bits=0, logup=True, max_apc_airs=2, periphery_layout="preprocessed")
    yield seg
    seg.close()


def test_the_workload_in_the_preprocessed_layout(gpu, workload):
    torch, prover, periphery = gpu
    from powdr_amd import segment_workload as sw

    plain = sw.HonestSegment("C4", max_log_height=9, seed=2, queries=4, pow_bits=0, logup=True, max_apc_airs=2)
    plain.generate_traces()
    plain_words = plain.prove(copy=True)
    assert plain_words[0] == MAGIC3 and plain.verify(plain_words) == 0
    seg = workload
    seg.generate_traces()
    pf = seg.prove(copy=True)
    assert pf[0] == MAGIC4
    assert seg.verify(pf) == 0 and seg.check_constraints() == 0
    assert seg.balance_witness()[0] == 0
    per = {a["name"]: a for a in seg.airs if a["role"] == "periphery"}
    assert [per[n]["width"] for n in ("var_range", "tuple2", "bitwise")] == [1, 1, 2]
    assert seg.cells_by_role["periphery"] == plain.cells_by_role["periphery"] - sum(
        (a["pre"][1] << a["log_h"]) for a in per.values())  # main cells only
    assert seg.cells_by_role["apc"] == plain.cells_by_role["apc"]
    # a second generation: the same words
    seg.generate_traces()
    assert (seg.prove(copy=True) == pf).all()
    # one histogram bin off by one: the lookup buses no longer balance
    seg.per.var_hist[5] += 1
    periphery.multiplicities(seg.per.var_hist, out=seg.per_traces["var_range"])
    assert seg.balance_witness()[0] == 14
    # the default layout's words did not move
    plain.generate_traces()
    assert (plain.prove(copy=True) == plain_words).all()
    plain.close()


def test_preprocessed_airs_stay_resident_while_others_stream(gpu, workload, monkeypatch):
    """Under a device budget apc0 streams with its trace handed over; the periphery AIRs (preprocessed) stay resident; same words."""
    torch, prover, _ = gpu
    seg = workload
    seg.generate_traces()
    want = seg.prove(copy=True)
    resident = prover.segment_last_plan()[0]
    monkeypatch.setenv("POWDR_STREAM_MIN_LOG_HEIGHT", "8")
    try:
        prover.set_device_budget(int(0.8 * resident))
        seg.generate_traces()
        got = seg.prove(copy=True, hand_over=True)
        modes = dict(zip([a["name"] for a in seg.airs], prover.segment_last_modes()))
    finally:
        prover.set_device_budget(0)
    assert (got == want).all()
    assert modes["apc0"][0] > 0 and modes["apc0"][1]
    assert all(modes[n] == (0, False) for n in ("var_range", "tuple2", "bitwise"))
    # forcing every AIR to stream leaves them resident as well
    monkeypatch.setenv("POWDR_STREAM_LOG_BLOCKS", "1")
    seg.generate_traces()
    assert (seg.prove(copy=True) == want).all()
    modes = dict(zip([a["name"] for a in seg.airs], prover.segment_last_modes()))
    assert all(modes[n][0] == 0 for n in ("var_range", "tuple2", "bitwise")) and modes["apc0"][0] == 1
