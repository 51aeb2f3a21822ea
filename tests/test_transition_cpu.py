"""pw-stark v1 + rows, the host side: pw_verify_segment_transition on segments without a row-aware AIR gives the
codes of pw_verify_segment, the operand bounds of the row layout, and the row layout in air_text. No GPU: the proofs come from the
oracle."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests.test_segment_proof import SPEC, descs_of, synthetic_airs

P = om.P


@pytest.fixture(scope="module", params=[False, True], ids=["constraints", "logup"])
def oracle_segment(request):
    logup = request.param
    airs = synthetic_airs(SPEC)
    return logup, airs, sm.prove_segment(airs, num_queries=5, pow_bits=4, logup=logup)


def test_plain_descriptions_give_the_codes_of_pw_verify_segment(oracle_segment):
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    none, zero = [None] * len(airs), [(0, np.zeros(8, np.uint32))] * len(airs)
    want_rc, want_total = prover.verify_segment(descs, pf, 5, 4, logup)
    for keys in (None, none, zero):
        rc, total = prover.verify_segment(descs, pf, 5, 4, logup, preprocessed=keys, transition=True)
        assert rc == want_rc == 0 and (total == want_total).all()
    rng = np.random.default_rng(11)
    codes = set()
    for pos in list(range(0, 24)) + [int(x) for x in rng.integers(24, len(pf), 40)] + [len(pf) - 1]:
        bad = pf.copy()
        bad[pos] = (int(bad[pos]) + 1 + int(rng.integers(0, 1000))) % P
        want = prover.verify_segment(descs, bad, 5, 4, logup)[0]
        assert want != 0
        assert prover.verify_segment(descs, bad, 5, 4, logup, transition=True)[0] == want, pos
        assert prover.verify_segment(descs, bad, 5, 4, logup, preprocessed=zero, transition=True)[0] == want, pos
        codes.add(want)
    assert len(codes) >= 3
    for cut in (pf[:-1], pf[:40], np.concatenate([pf, pf[:1]])):
        assert prover.verify_segment(descs, cut, 5, 4, logup, transition=True)[0] == prover.verify_segment(descs, cut, 5, 4, logup)[0]


def _with_constraint(desc, code):
    """desc with its first constraint replaced by `code` (post-fix, appended to the bytecode)."""
    W, lh, bc, sp, it = desc
    bc = np.asarray(bc, np.uint32)
    new_sp = np.asarray(sp, np.uint32).reshape(-1, 2).copy()
    new_sp[0] = (len(bc), len(code))
    return (W, lh, np.concatenate([bc, np.asarray(code, np.uint32)]), new_sp, it)


def test_row_aware_descriptions_against_a_pws3_proof(oracle_segment):
    """A description that reads the next row or a selector makes its AIR row-aware: against a PWS3 proof the header does not
    match (1). The same descriptions are malformed (15) for the verifiers without the row layout."""
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    W = descs[1][0]
    rows = prover.row_operands(W)
    for operand in (rows.next(0), rows.next(W - 1), rows.is_first_row, rows.is_last_row, rows.is_transition):
        bad = list(descs)
        bad[1] = _with_constraint(descs[1], [om.OP_PUSH_APC, operand])
        assert prover.verify_segment(bad, pf, 5, 4, logup, transition=True)[0] == 1
        assert prover.verify_segment(bad, pf, 5, 4, logup)[0] == 15
        assert prover.verify_segment(bad, pf, 5, 4, logup, preprocessed=[None] * len(airs))[0] == 15


def test_operands_past_the_row_layout_are_malformed(oracle_segment):
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    W = descs[1][0]
    rows = prover.row_operands(W)
    for operand in (rows.bound, rows.bound + 1, 0xffffffff):
        bad = list(descs)
        bad[1] = _with_constraint(descs[1], [om.OP_PUSH_APC, operand])
        assert prover.verify_segment(bad, pf, 5, 4, logup, transition=True)[0] == 15
    # the bound follows the preprocessed width: 2 (W + 1) + 2 is is_transition with one preprocessed column, past the end without
    keys = [None] * len(airs)
    keys[1] = (1, np.arange(8, dtype=np.uint32))
    bad = list(descs)
    bad[1] = _with_constraint(descs[1], [om.OP_PUSH_APC, 2 * (W + 1) + 2])
    assert prover.verify_segment(bad, pf, 5, 4, logup, transition=True)[0] == 15
    assert prover.verify_segment(bad, pf, 5, 4, logup, preprocessed=keys, transition=True)[0] == 1


def test_next_row_and_selector_operands_in_interactions_are_malformed():
    from powdr_amd import prover

    airs = synthetic_airs(SPEC)
    pf = sm.prove_segment(airs, num_queries=5, pow_bits=4, logup=True)
    descs = descs_of(airs)
    W, lh, bc, sp, (it, isp, ibc) = descs[1]
    rows = prover.row_operands(W)
    assert prover.verify_segment(descs, pf, 5, 4, True, transition=True)[0] == 0
    for operand in (rows.next(0), rows.is_first_row, rows.is_last_row, rows.is_transition):
        ibc2 = np.concatenate([np.asarray(ibc, np.uint32), np.array([om.OP_PUSH_APC, operand], np.uint32)])
        isp2 = np.asarray(isp, np.uint32).reshape(-1, 2).copy()
        isp2[int(it[0][2]) + 1] = (len(ibc), 2)  # the first argument of the first interaction
        bad = list(descs)
        bad[1] = (W, lh, bc, sp, (it, isp2, ibc2))
        assert prover.verify_segment(bad, pf, 5, 4, True, transition=True)[0] == 15


def test_air_text_row_layout():
    from powdr_amd.air_text import compile_expr
    from powdr_amd.prover import row_operands

    col = {"a": 0, "b": 1, "s": 2, "d": 3, "x": 4}
    rows = row_operands(5)
    PC, K, ADD, SUB, MUL = om.OP_PUSH_APC, om.OP_PUSH_CONST, 2, 3, 4
    assert compile_expr("a' - b", col, rows) == [PC, rows.next(0), PC, 1, SUB]
    assert compile_expr("is_first_row * (x - 1)", col, rows) == [PC, rows.is_first_row, PC, 4, K, 1, SUB, MUL]
    assert compile_expr("is_transition * (s' - s - d)", col, rows) == [PC, rows.is_transition, PC, rows.next(2), PC, 2, SUB, PC, 3, SUB, MUL]
    assert compile_expr("is_last_row * b'", col, rows) == [PC, rows.is_last_row, PC, rows.next(1), MUL]
    assert (rows.next(0), rows.is_first_row, rows.is_last_row, rows.is_transition, rows.bound) == (5, 10, 11, 12, 13)
    assert row_operands(5, 2).is_transition == 2 * 7 + 2
    # without the layout: rejected, as before
    for text in ("a' - b", "is_first_row * (x - 1)", "is_transition * (s' - s - d)", "is_last_row"):
        with pytest.raises(ValueError):
            compile_expr(text, col)
    # a column named like a selector stays that column
    assert compile_expr("is_transition", {"is_transition": 3}, rows) == [PC, 3]
    with pytest.raises(ValueError):
        compile_expr("q'", col, rows)  # unknown column


def test_rust_binds_the_row_layout_entries():
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name in ("pw_prover_create_transition", "pw_prover_row_flags", "pw_verify_segment_transition"):
        assert name in c and r.get(name) == c[name]
