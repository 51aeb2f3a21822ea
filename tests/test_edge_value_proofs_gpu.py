"""Edge-valued traces (tests/_edge_values.py: the table test_edge_values_cpu.py validates) PROVED on the device, on every expression
path, against the oracle: constant columns of extreme canonical values and extreme Montgomery words put an accumulator's terms at
their bound on the whole extended domain, on every column and on consecutive rows at once — what a random trace never does. Exact
field arithmetic: the proof words are the oracle's, whatever the path; the verifiers answer what the CPU table holds.

  interp      POWDR_JIT=0: the xbc interpreter kernels (quotient_kernel / quotient_logup_kernel, logup_perm_kernel with the small forms)
  postfix     + POWDR_QUOTIENT_XBC=0, POWDR_LOGUP_INTERPRET=1: the post-fix interpreter, the LogUp programs interpreted
  jit         POWDR_JIT=1: the run-time specialised kernels
  streamed    POWDR_JIT=0, POWDR_STREAM_LOG_BLOCKS=2: the sub-coset path (ext_dot_partial_kernel's openings, the DEEP numerator as a
              polynomial); heights of at least 2^3 rows
  deep_direct 2^16 rows (`hand`): the DEEP combination on the un-extended matrices, and deep_kernel over the LDE with POWDR_DEEP_DIRECT=1

The oracle's proofs are made once per (AIR, height, kind) and shared by the paths."""
import functools

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _edge_values as ev

P = ev.P
NQ, PB = ev.NUM_QUERIES, ev.POW_BITS

PATH_ENV = {
    "interp": {"POWDR_JIT": "0"},
    "postfix": {"POWDR_JIT": "0", "POWDR_QUOTIENT_XBC": "0", "POWDR_LOGUP_INTERPRET": "1"},
    "jit": {"POWDR_JIT": "1"},
    "streamed": {"POWDR_JIT": "0", "POWDR_STREAM_LOG_BLOCKS": "2"},
}
_ALL_ENV = ["POWDR_JIT", "POWDR_QUOTIENT_XBC", "POWDR_LOGUP_INTERPRET", "POWDR_STREAM_LOG_BLOCKS", "POWDR_DEEP_DIRECT"]
PROOF_CASES = [(air, log_h, path) for air, log_h in ev.CASES for path in PATH_ENV if path != "streamed" or log_h >= 3]


def _is_slow(air, log_h, path):
    """2^13 rows (the oracle's share of a case: 4 s for `one` to 9 s for `wide`) runs with POWDR_RUN_SLOW=1, except `hand` on the
    interpreter path, which keeps the second chunk of the LogUp prefix scan in every run; 2^12 rows and the short heights always run."""
    return log_h == 13 and (air, path) != ("hand", "interp")


def _params(cases, slow, ident):
    return [pytest.param(*c, id=ident(*c), marks=[pytest.mark.slow] if slow(*c) else []) for c in cases]


@pytest.fixture(scope="module")
def gpu():
    import torch
    from powdr_amd import abi, prover

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    return torch, abi, prover


def to_dev(torch, a):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(a, dtype=np.uint32)).view(np.int32)).cuda()


def _set_path(monkeypatch, path):
    for k in _ALL_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)


@functools.lru_cache(maxsize=None)
def _oracle_proof(air, kind, log_h, logup):
    """the oracle's proof of one table entry (read-only: shared by the paths)"""
    W, (bc, spans), it = ev.air_tables(air)
    flat = ev.trace(air, kind, log_h)
    pf = sm.prove_logup(flat, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB) if logup else sm.prove(flat, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)
    pf.setflags(write=False)
    return pf


def _same_words(got, want, what):
    assert len(got) == len(want), f"{what}: {len(got)} words, the oracle {len(want)}"
    assert (got == want).all(), f"{what}: first differing word {int(np.argmax(got != want))} of {len(want)}"


@functools.lru_cache(maxsize=None)
def _verifier_codes(air, kind, log_h, logup):
    """(the product's host verifier, the oracle's verifier) on the oracle's proof words: asked once per table entry, the paths share it"""
    from powdr_amd import prover

    W, (bc, spans), it = ev.air_tables(air)
    pf = _oracle_proof(air, kind, log_h, logup)
    if logup:
        return (prover.verify_logup(pf, W, log_h, bc, spans, it, num_queries=NQ, pow_bits=PB)[0],
                sm.verify_logup(pf, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB))
    return prover.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB), sm.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)


def _verifiers_answer(got, air, kind, log_h, logup, what):
    """prover.verify* and sm.verify* on the device's proof return the table's code. The verifiers are functions of the proof words, and
    `got` has just been found equal to the oracle's words, so their answers are taken once per table entry and not once per path."""
    assert got.shape == _oracle_proof(air, kind, log_h, logup).shape and (got == _oracle_proof(air, kind, log_h, logup)).all(), what
    code = ev.expected_code(air, kind, log_h)
    assert _verifier_codes(air, kind, log_h, logup) == (code, code), what


@pytest.mark.gpu
@pytest.mark.parametrize("air,log_h,path", _params(PROOF_CASES, _is_slow, lambda a, h, p: f"{a}-{h}-{p}"))
def test_edge_traces_prove_to_the_oracles_words_on_every_path(gpu, monkeypatch, air, log_h, path):
    """For every trace kind of the table, constraints-only and with LogUp: the proof words equal the oracle's, a second proof from
    the same prover is identical, both verifiers return the code the CPU table holds, and the path forced is the path taken."""
    torch, abi, prover = gpu
    W, (bc, spans), it = ev.air_tables(air)
    _set_path(monkeypatch, path)
    for logup in (False, True):
        pr = prover.Prover(W, bc, spans, num_queries=NQ, pow_bits=PB, interactions=it if logup else None)
        if path == "postfix" and logup:
            assert pr.logup_path() == 1
        if path == "streamed":
            assert pr.stream_log_blocks(log_h) >= 1  # at least one sub-coset level at this height
        # nothing to specialise in an AIR without constraints and without interactions (`one`, constraints-only): the prover says
        # so (state -1) and its empty quotient stays with the interpreter kernel
        nothing_to_specialise = len(spans) == 0 and not logup
        for kind in ev.kinds(air):
            what = f"{air} 2^{log_h} {path} {'LogUp' if logup else 'constraints only'} {kind}"
            d_t = to_dev(torch, ev.trace(air, kind, log_h))
            abi.call_stats(reset=True)
            got = pr.prove(d_t.data_ptr(), log_h)
            st = abi.call_stats()
            if path == "jit" and not nothing_to_specialise:
                assert pr.specialised()["state"] == 1, (what, pr.specialised())
                assert st["jit_launches"] >= 1 and st["interpreter_launches"] == 0, (what, st)
            elif path == "jit":
                assert pr.specialised()["state"] == -1 and st["jit_launches"] == 0, (what, pr.specialised(), st)
            else:
                assert st["interpreter_launches"] >= 1 and st["jit_launches"] == 0, (what, st)
            _same_words(got, _oracle_proof(air, kind, log_h, logup), what)
            assert (pr.prove(d_t.data_ptr(), log_h) == got).all(), f"{what}: the second proof differs"
            _verifiers_answer(got, air, kind, log_h, logup, what)
            del d_t
        pr.close()


# the DEEP combination on the un-extended matrices (from 2^16 rows on) and deep_kernel over the LDE at the same height
DEEP_KINDS = ev.kinds("hand")
DEEP_KINDS_ALWAYS = ("const[word(p-1)]", "cells", "runs4")  # (3 to 4 s each, most of it the oracle's; the others: POWDR_RUN_SLOW=1)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", _params([(k,) for k in DEEP_KINDS], lambda k: k not in DEEP_KINDS_ALWAYS, lambda k: k))
def test_deep_combination_at_2_to_16_rows_both_forms(gpu, monkeypatch, kind):
    """`hand` at 2^16 rows, one trace kind per case (the oracle needs seconds per proof here): the default form (the DEEP numerator
    combined on the un-extended matrices and extended) and POWDR_DEEP_DIRECT=1 (deep_kernel / deep_logup_kernel over the LDE of every
    column) both give the oracle's words."""
    torch, abi, prover = gpu
    air, log_h = "hand", ev.DEEP_COMBO_LOG_HEIGHT
    W, (bc, spans), it = ev.air_tables(air)
    _set_path(monkeypatch, "interp")
    d_t = to_dev(torch, ev.trace(air, kind, log_h))
    assert d_t.data_ptr() % 8 == 0  # (the combination reads 8-byte pairs; a misaligned trace would take deep_kernel silently)
    for logup in (False, True):
        want = _oracle_proof(air, kind, log_h, logup)
        pr = prover.Prover(W, bc, spans, num_queries=NQ, pow_bits=PB, interactions=it if logup else None)
        assert pr.stream_log_blocks(log_h) == 0  # resident: the streamed path has a DEEP stage of its own
        for direct in (False, True):
            what = f"hand 2^16 {'LogUp' if logup else 'constraints only'} {kind} {'POWDR_DEEP_DIRECT=1' if direct else 'combined un-extended'}"
            if direct:
                monkeypatch.setenv("POWDR_DEEP_DIRECT", "1")
            else:
                monkeypatch.delenv("POWDR_DEEP_DIRECT", raising=False)
            got = pr.prove(d_t.data_ptr(), log_h)
            _same_words(got, want, what)
            assert (pr.prove(d_t.data_ptr(), log_h) == got).all(), f"{what}: the second proof differs"
        monkeypatch.delenv("POWDR_DEEP_DIRECT", raising=False)
        _verifiers_answer(got, air, kind, log_h, logup, what)
        pr.close()


# ---------------------------------------------------------------------------------------------------------------- one segment
SEGMENT_AIRS = [("hand", 8), ("wide", 12), ("one", 1)]
SEGMENT_KINDS = ["const[word(p-1)]", "cells", "runs4", "all_padding", "const[0]"]  # (const[0]: the kind every AIR is satisfied on)


def _segment_airs(kind):
    out = []
    for air, log_h in SEGMENT_AIRS:
        W, (bc, spans), it = ev.air_tables(air)
        out.append((ev.trace(air, kind, log_h), W, log_h, bc, spans, it))
    return out


@functools.lru_cache(maxsize=None)
def _oracle_segment_proof(kind, logup):
    pf = sm.prove_segment(_segment_airs(kind), num_queries=NQ, pow_bits=PB, logup=logup)
    pf.setflags(write=False)
    return pf


@pytest.mark.gpu
@pytest.mark.parametrize("jit", ["0", "1"])
@pytest.mark.parametrize("logup", [False, True])
def test_segment_of_edge_traces(gpu, monkeypatch, logup, jit):
    """`hand` at 2^8, `wide` at 2^12 and `one` at 2^1 rows in ONE segment proof: the oracle's words; the product's segment verifier
    accepts exactly where the CPU table says every AIR is satisfied, and otherwise names an AIR the table says is not."""
    torch, abi, prover = gpu
    _set_path(monkeypatch, "jit" if jit == "1" else "interp")
    tables = [ev.air_tables(air) for air, _ in SEGMENT_AIRS]
    provers = [prover.Prover(W, bc, spans, num_queries=NQ, pow_bits=PB, interactions=it if logup else None) for W, (bc, spans), it in tables]
    descs = [(W, log_h, bc, spans, it if logup else None) for (W, (bc, spans), it), (_, log_h) in zip(tables, SEGMENT_AIRS)]
    for kind in SEGMENT_KINDS:
        what = f"segment, {'LogUp' if logup else 'constraints only'}, POWDR_JIT={jit}, {kind}"
        airs = _segment_airs(kind)
        traces = [to_dev(torch, a[0]) for a in airs]
        abi.call_stats(reset=True)
        got = prover.prove_segment([(pr, t.data_ptr(), a[2]) for pr, t, a in zip(provers, traces, airs)], logup=logup)
        st = abi.call_stats()
        assert (st["jit_launches"] > 0) == (jit == "1"), (what, st)
        _same_words(got, _oracle_segment_proof(kind, logup), what)
        codes = [ev.expected_code(air, kind, log_h) for air, log_h in SEGMENT_AIRS]
        rc = prover.verify_segment(descs, got, NQ, PB, logup)[0]
        assert (rc == 0) == all(c == 0 for c in codes), (what, rc, codes)
        if rc:  # ((i + 1) << 8) | 2: the constraint identity of AIR i
            assert rc & 0xFF == 2 and codes[(rc >> 8) - 1] == 2, (what, rc, codes)
        assert sm.verify_segment(got, airs, num_queries=NQ, pow_bits=PB, logup=logup)[0] == rc, what
    assert all(c == 0 for c in (ev.expected_code(air, "const[0]", log_h) for air, log_h in SEGMENT_AIRS))  # (the accepting case exists)
    for pr in provers:
        pr.close()


# ---------------------------------------------------------------------------------------------------------------- mock prover
@pytest.mark.gpu
@pytest.mark.parametrize("path", ["interp", "postfix"])
def test_mock_prover_locates_a_corrupted_cell_at_the_edges(gpu, monkeypatch, path):
    """pw_prover_check_constraints where test_mock_prover_reports_violations does not look: the satisfied edge trace has no violation;
    one cell of column 3 set to word(p-1) at row 0, 255, 256 (a workgroup's last lane, the next one's first) or H-1 is reported at
    that row, with the constraint the plain-integer evaluator names as the first non-zero one."""
    torch, abi, prover = gpu
    air, log_h = "hand", 12
    W, (bc, spans), it = ev.air_tables(air)
    H = 1 << log_h
    _set_path(monkeypatch, path)
    pr = prover.Prover(W, bc, spans, num_queries=2)
    flat = ev.trace(air, "satisfied", log_h)
    assert ev.first_violation(air, flat) is None
    d_t = to_dev(torch, flat)
    assert pr.check_constraints(d_t.data_ptr(), log_h) == (0, None, None)
    bad = ev.word(P - 1)
    bad_m = int(om.to_monty(np.array([bad], np.uint32))[0])
    assert bad_m == P - 1
    for row in (0, 255, 256, H - 1):
        corrupt = flat.copy()
        assert int(corrupt[3 * H + row]) != bad
        corrupt[3 * H + row] = bad
        want = ev.first_violation(air, corrupt)
        assert want is not None and want[0] == row
        d_c = d_t.clone()
        d_c[3 * H + row] = bad_m
        n, got_row, got_c = pr.check_constraints(d_c.data_ptr(), log_h)
        assert n >= 1 and (got_row, got_c) == want, (row, n, got_row, got_c, want)
    assert pr.check_constraints(d_t.data_ptr(), log_h) == (0, None, None)
    pr.close()
