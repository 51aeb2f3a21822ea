"""Random AIRs (tests/_random_airs.py) PROVED on the device, on every expression path, against the oracle and against the generator's
own integer evaluation. The seed lists, their heights and trace kinds are test_random_airs_cpu.py's, whose census says what they
contain (every planted shape, the depth-15/16 chains, groups of three and more, W across the 64-column tile, ...).

  interp      POWDR_JIT=0: the xbc interpreter kernels (quotient_kernel / quotient_logup_kernel, logup_perm_kernel with the small forms)
  postfix     + POWDR_QUOTIENT_XBC=0, POWDR_LOGUP_INTERPRET=1: the post-fix interpreter, the LogUp programs interpreted
  jit         POWDR_JIT=1: the run-time specialised kernels; with POWDR_JIT_CHUNK_COST=200 POWDR_JIT_UNIT_CHUNKS=1 several chunks and
              translation units per AIR, so that the combine kernels run after several specialised launches
  streamed    POWDR_JIT=0, POWDR_STREAM_LOG_BLOCKS=2: the sub-coset path; heights of at least 2^3 rows

The oracle's proofs are made once per (seed, kind of proof) and shared by the paths."""
import functools

import numpy as np
import pytest

from oracle import stark_model as sm
from tests import _random_airs as ra
from tests import test_random_airs_cpu as lists
from tests.test_edge_value_proofs_gpu import PATH_ENV, _ALL_ENV, _same_words, to_dev

P = ra.P
NQ, PB = 4, 0
_CHUNK_ENV = ["POWDR_JIT_CHUNK_COST", "POWDR_JIT_UNIT_CHUNKS"]
NO_INTER = (np.zeros((0, 3), np.uint32), np.zeros((0, 2), np.uint32), np.zeros(0, np.uint32))


@pytest.fixture(scope="module")
def gpu():
    import torch
    from powdr_amd import abi, prover

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    return torch, abi, prover


def _set_path(monkeypatch, path, small_chunks=False):
    for k in _ALL_ENV + _CHUNK_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)
    if small_chunks:
        monkeypatch.setenv("POWDR_JIT_CHUNK_COST", "200")
        monkeypatch.setenv("POWDR_JIT_UNIT_CHUNKS", "1")


@functools.lru_cache(maxsize=None)
def _air(seed):
    return ra.random_air(seed)


@functools.lru_cache(maxsize=None)
def _flat(seed):
    t = ra.trace(_air(seed)[3], lists.proof_log_height(seed), lists.proof_trace_kind(seed))
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _oracle_proof(seed, logup):
    """the oracle's proof of one seed (read-only: shared by the paths)"""
    W, (bc, spans), it, _ = _air(seed)
    log_h = lists.proof_log_height(seed)
    pf = (sm.prove_logup(_flat(seed), W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB) if logup else
          sm.prove(_flat(seed), W, log_h, bc, spans, num_queries=NQ, pow_bits=PB))
    pf.setflags(write=False)
    return pf


@functools.lru_cache(maxsize=None)
def _expected_code(seed):
    """0 where the generator's evaluation finds every constraint satisfied on every row, else 2 (the constraint identity)"""
    meta = _air(seed)[3]
    return 0 if ra.violations(meta["constraints"], np.asarray(_flat(seed)).reshape(meta["W"], -1))[1] == 0 else 2


@functools.lru_cache(maxsize=None)
def _verifier_codes(seed, logup):
    from powdr_amd import prover

    W, (bc, spans), it, _ = _air(seed)
    log_h, pf = lists.proof_log_height(seed), _oracle_proof(seed, logup)
    if logup:
        return (prover.verify_logup(pf, W, log_h, bc, spans, it, num_queries=NQ, pow_bits=PB)[0],
                sm.verify_logup(pf, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB))
    return prover.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB), sm.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)


def _prove_one_air(gpu, seed, path):
    """constraints only and (an AIR with interactions) with LogUp: the words are the oracle's, a second proof is identical, the path
    forced is the path taken; -> [specialised()] of the provers (jit)"""
    torch, abi, prover = gpu
    W, (bc, spans), it, meta = _air(seed)
    log_h = lists.proof_log_height(seed)
    d_t = to_dev(torch, _flat(seed))
    out = []
    for logup in ([False, True] if len(it[0]) else [False]):
        what = f"seed {seed} 2^{log_h} {path} {'LogUp' if logup else 'constraints only'}"
        pr = prover.Prover(W, bc, spans, num_queries=NQ, pow_bits=PB, interactions=it if logup else None)
        if path == "postfix" and logup:
            assert pr.logup_path() == 1
        if path == "streamed":
            assert pr.stream_log_blocks(log_h) >= 1
        nothing_to_specialise = len(spans) == 0 and not logup
        abi.call_stats(reset=True)
        got = pr.prove(d_t.data_ptr(), log_h)
        st = abi.call_stats()
        if path == "jit" and not nothing_to_specialise:
            assert pr.specialised()["state"] == 1, (what, pr.specialised())
            assert st["jit_launches"] >= 1 and st["interpreter_launches"] == 0, (what, st)
            out.append(dict(pr.specialised(), logup=logup))
        elif path == "jit":
            assert pr.specialised()["state"] == -1 and st["jit_launches"] == 0, (what, pr.specialised(), st)
        else:
            assert st["interpreter_launches"] >= 1 and st["jit_launches"] == 0, (what, st)
        _same_words(got, _oracle_proof(seed, logup), what)
        assert (pr.prove(d_t.data_ptr(), log_h) == got).all(), f"{what}: the second proof differs"
        assert _verifier_codes(seed, logup) == (_expected_code(seed),) * 2, what
        pr.close()
    return out


PROOF_CASES = [(s, p) for s in lists.PROOF_SEEDS for p in ("interp", "postfix", "streamed") if p != "streamed" or lists.proof_log_height(s) >= 3]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,path", PROOF_CASES, ids=[f"{s}-{p}" for s, p in PROOF_CASES])
def test_random_airs_prove_to_the_oracles_words(gpu, monkeypatch, seed, path):
    """24 random AIRs at 2^1 .. 2^6 rows (two at 2^12: the fused LDE schedule; one at 2^13: the LogUp prefix scan crosses its 4096-row
    block) on the interpreter paths and streamed: sm.prove's / sm.prove_logup's words."""
    _set_path(monkeypatch, path)
    _prove_one_air(gpu, seed, path)


@pytest.mark.gpu
@pytest.mark.parametrize("small_chunks", [False, True], ids=["default_chunking", "chunk_cost_200_one_chunk_per_unit"])
@pytest.mark.parametrize("seed", lists.JIT_SEEDS)
def test_random_airs_prove_to_the_oracles_words_specialised(gpu, monkeypatch, seed, small_chunks):
    """The run-time specialised kernels of 8 of the seeds (the depth-16 chains, groups of three and more), with the default chunking and
    cut into several chunks of one translation unit each: a chunk boundary falls between two constraints and inside a LogUp group's
    neighbourhood, the partial-sum buffers, quotient_logup_tail_kernel and rowsum_combine_kernel run after several specialised launches."""
    torch, abi, prover = gpu
    _set_path(monkeypatch, "jit", small_chunks)
    W, (bc, spans), it, meta = _air(seed)
    specs = _prove_one_air(gpu, seed, "jit")
    print(f"seed {seed} small_chunks={small_chunks}: " + "; ".join(f"{'LogUp' if s['logup'] else 'constraints'}: {s['kernels']} kernels, {s['chunks']} chunks" for s in specs))
    assert len(specs) == 2
    if small_chunks:
        # what the generator makes of these parameters on the host: several chunks for both kernel families
        totals = [prover.jit_generated_sources(W, bc, spans, it, which, 200, 1)[1] for which in (0, 1)]
        assert min(totals) >= 2, totals
        s = specs[1]  # (one chunk per unit: as many kernels as chunks, the quotient's and the permutation columns' together)
        assert s["kernels"] == s["chunks"] == sum(totals), (s, totals)
        alone = prover.jit_generated_sources(W, bc, spans, None, 0, 200, 1)[1]
        assert specs[0]["kernels"] == specs[0]["chunks"] == alone, (specs[0], alone)


# ---------------------------------------------------------------------------------------------------------------- one segment
@functools.lru_cache(maxsize=None)
def _segment(seed):
    return lists.segment_airs(seed)


@functools.lru_cache(maxsize=None)
def _oracle_segment_proof(seed, logup):
    pf = sm.prove_segment(_segment(seed), num_queries=NQ, pow_bits=PB, logup=logup)
    pf.setflags(write=False)
    return pf


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["interp", "jit"])
@pytest.mark.parametrize("logup", [False, True], ids=["constraints", "logup"])
@pytest.mark.parametrize("seed", lists.SEGMENT_SEEDS)
def test_segments_of_random_airs(gpu, monkeypatch, seed, logup, path):
    """three random AIRs of different heights in ONE segment proof: sm.prove_segment's words; both segment verifiers answer alike"""
    torch, abi, prover = gpu
    _set_path(monkeypatch, path)
    airs = _segment(seed)
    tables = [(it if it is not None else NO_INTER) if logup else None for *_, it in airs]
    provers = [prover.Prover(W, bc, spans, num_queries=NQ, pow_bits=PB, interactions=t) for (_, W, _, bc, spans, _), t in zip(airs, tables)]
    traces = [to_dev(torch, a[0]) for a in airs]
    abi.call_stats(reset=True)
    got = prover.prove_segment([(pr, t.data_ptr(), a[2]) for pr, t, a in zip(provers, traces, airs)], logup=logup)
    st = abi.call_stats()
    something = any(len(a[4]) or (logup and a[5] is not None) for a in airs)
    assert (st["jit_launches"] > 0) == (path == "jit" and something), st
    _same_words(got, _oracle_segment_proof(seed, logup), f"segment {seed} logup={logup} {path}")
    rc = prover.verify_segment([(a[1], a[2], a[3], a[4], t) for a, t in zip(airs, tables)], got, NQ, PB, logup)[0]
    assert sm.verify_segment(got, airs, num_queries=NQ, pow_bits=PB, logup=logup)[0] == rc
    clean = [ra.violations(ra.random_air(3 * seed + k)[3]["constraints"], np.asarray(a[0]).reshape(a[1], -1))[1] == 0 for k, a in enumerate(airs)]
    assert rc == (0 if all(clean) else ((clean.index(False) + 1) << 8) | 2), (rc, clean)
    for pr in provers:
        pr.close()


# ---------------------------------------------------------------------------------------------------------------- mock prover
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["interp", "postfix"])
@pytest.mark.parametrize("seed", lists.MOCK_SEEDS)
def test_mock_prover_counts_and_locates_what_the_generator_does(gpu, monkeypatch, seed, path):
    """check_constraints on a trace whose last third is zero rows (clean for the homogeneous AIRs): the number of violated
    (row, constraint) pairs and the first of them in row-major order are the generator's."""
    torch, abi, prover = gpu
    _set_path(monkeypatch, path)
    W, (bc, spans), it, meta = _air(seed)
    T = ra.trace_matrix(meta, lists.MOCK_LOG_HEIGHT, "zero_rows")
    pairs, rows, first = ra.violations(meta["constraints"], T)
    pr = prover.Prover(W, bc, spans, num_queries=2)
    d_t = to_dev(torch, T.reshape(-1))
    got = pr.check_constraints(d_t.data_ptr(), lists.MOCK_LOG_HEIGHT)
    assert got == ((pairs,) + first if pairs else (0, None, None)), (got, pairs, rows, first)
    pr.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["interp", "postfix"])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_bus_check_of_a_derived_air(gpu, monkeypatch, seed, path):
    """check_segment_buses with tally_all on an AIR whose bus balances by construction: balanced; after one changed argument cell of a
    receive, the two tuples the generator's tally leaves (the send without its receive, the receive of a tuple nobody sent)."""
    torch, abi, prover = gpu
    _set_path(monkeypatch, path)
    d = ra.derived_air(seed, 5)
    H = 1 << d["log_h"]
    pr = prover.Prover(d["W"], *d["cons"], num_queries=2, interactions=d["it"])
    d_t = to_dev(torch, d["T"].reshape(-1))
    n_active = H * len(d["interactions"])
    summaries, tuples = prover.check_segment_buses([(pr, d_t.data_ptr(), d["log_h"])], tally_all=True)
    assert summaries == [dict(bus=ra.DERIVED_BUS, status=0, n_active=n_active, n_unbalanced=0)] and tuples == []
    bad = d["T"].copy()
    r = 7
    bad[d["W"] - 1, r] = (int(bad[d["W"] - 1, r]) + 1) % P  # the last column: the last argument of the last receive
    want = ra.bus_tally(d["interactions"], bad)
    assert len(want) == 2 and sorted(want.values()) == [1, P - 1]
    d_b = to_dev(torch, bad.reshape(-1))
    summaries, tuples = prover.check_segment_buses([(pr, d_b.data_ptr(), d["log_h"])], tally_all=True)
    assert summaries == [dict(bus=ra.DERIVED_BUS, status=1, n_active=n_active, n_unbalanced=2)]
    assert {(t["bus"], tuple(t["args"])): t["net_multiplicity"] for t in tuples} == want
    assert all(t["n_contributions"] == 1 and t["n_args"] == len(t["args"]) for t in tuples)
    assert [(t["air"], t["interaction"], t["row"]) for t in tuples if t["net_multiplicity"] == P - 1] == [(0, len(d["interactions"]) - 1, r)]
    pr.close()


# ---------------------------------------------------------------------------------------------------------------- row-aware AIRs
@pytest.mark.gpu
@pytest.mark.parametrize("seed", lists.ROW_AWARE_SEEDS)
def test_row_aware_derived_airs(gpu, monkeypatch, seed):
    """derived_air(row_aware=True) - next-row reads under is_transition, is_first_row / is_last_row, preprocessed columns, public values -
    in a segment proof at 2^2 .. 2^5 rows. No byte oracle speaks this layout: (a) the mock prover finds the trace clean, (b) interp,
    postfix and jit give identical words, (c) the host verifier accepts with a balanced bus, (d) one changed derived cell is named by the
    mock prover as the generator's evaluation names it and its proof is rejected with code 2, (e) a wrong public value is rejected."""
    torch, abi, prover = gpu
    log_h = 2 + seed % 4
    d = ra.derived_air(seed, log_h, row_aware=True)
    W, n_pub = d["W"], len(d["public"])
    desc = [(W, log_h, *d["cons"], d["it"])]
    d_t = to_dev(torch, d["T"].reshape(-1))
    mode, j = [k for k in d["kinds"] if k[0] in ("row", "next", "fixed")][seed % 2]
    bad = d["T"].copy()
    r = (1 << log_h) // 2
    bad[j, r] = (int(bad[j, r]) + 1) % P
    want_bad = d["check"](bad)
    assert want_bad[1] >= 1 and want_bad[2][0] in (r - 1, r)
    d_b = to_dev(torch, bad.reshape(-1))
    wrong = d["public"].copy()
    wrong[0] = (int(wrong[0]) + 1) % P
    want_wrong = d["check"](d["T"], wrong)
    assert want_wrong[2] == (0, len(d["constraints"]) - 2)
    words = {}
    for path in ("interp", "postfix", "jit"):
        _set_path(monkeypatch, path)
        pr = prover.Prover(W, *d["cons"], num_queries=NQ, pow_bits=PB, interactions=d["it"], preprocessed=(to_dev(torch, d["pre"].reshape(-1)), d["pre_width"], log_h),
                           transition=True, n_public=n_pub)
        key = [(d["pre_width"], pr.preprocessed_root())]
        assert pr.row_flags == 3
        pr.set_public_values(d["public"])
        assert pr.check_constraints(d_t.data_ptr(), log_h) == (0, None, None)                                    # (a)
        abi.call_stats(reset=True)
        words[path] = prover.prove_segment([(pr, d_t.data_ptr(), log_h)], logup=True)
        st = abi.call_stats()
        assert (st["jit_launches"] > 0) == (path == "jit") and (path != "jit" or pr.specialised()["state"] == 1), (path, st)
        if path == "postfix":
            assert pr.logup_path() == 1
        verify = lambda pf, public: prover.verify_segment(desc, pf, NQ, PB, True, check_balance=True, preprocessed=key, transition=True, public=public)[0]
        assert verify(words[path], [d["public"]]) == 0                                                           # (c)
        assert verify(words[path], [wrong]) == 17                                                                # (e): not the expected values
        n, row, c = pr.check_constraints(d_b.data_ptr(), log_h)                                                  # (d)
        assert (n, (row, c)) == (want_bad[0], want_bad[2]), (path, n, row, c, want_bad)
        rc = verify(prover.prove_segment([(pr, d_b.data_ptr(), log_h)], logup=True), [d["public"]])
        assert rc == (1 << 8) | 2, (path, rc)
        pr.set_public_values(wrong)                                                                              # (e): proved with it
        n, row, c = pr.check_constraints(d_t.data_ptr(), log_h)
        assert (n, (row, c)) == (want_wrong[0], want_wrong[2]), (path, n, row, c, want_wrong)
        assert verify(prover.prove_segment([(pr, d_t.data_ptr(), log_h)], logup=True), [n_pub]) == (1 << 8) | 2
        pr.close()
    assert (words["interp"] == words["postfix"]).all() and (words["interp"] == words["jit"]).all()               # (b)


# ---------------------------------------------------------------------------------------------------------------- depth boundary
@pytest.mark.gpu
@pytest.mark.parametrize("kind", lists.SPAN_KINDS)
def test_depth_17_gets_no_prover(gpu, kind):
    """one slot past the evaluation stack (the depth-16 chains run inside the seeds above): creation refuses, nothing is launched"""
    torch, abi, prover = gpu
    (bc, spans), it = lists._planted(kind, lists.MALFORMED["depth17"])
    abi.call_stats(reset=True)
    with pytest.raises(RuntimeError):
        prover.Prover(lists.MW, bc, spans, num_queries=NQ, interactions=it)
    if kind == "constraint":
        with pytest.raises(RuntimeError):
            prover.Prover(lists.MW, bc, spans, num_queries=NQ)
    st = abi.call_stats()
    assert st["jit_launches"] == 0 and st["interpreter_launches"] == 0, st
    (bc, spans), it = lists._planted(kind, lists._chain_words(16))
    prover.Prover(lists.MW, bc, spans, num_queries=NQ, interactions=it).close()
