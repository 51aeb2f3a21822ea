"""pw-stark v1 + preprocessed columns, the host side: pw_verify_segment_preprocessed with every width 0 is
pw_verify_segment, a PWS3 proof is not accepted against a description that claims preprocessed columns, and program operands are
checked against the combined bound. No GPU: the proofs come from the oracle."""
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


def test_zero_widths_give_the_codes_of_pw_verify_segment(oracle_segment):
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    none = [None] * len(airs)
    zero = [(0, np.zeros(8, np.uint32))] * len(airs)
    for keys in (none, zero):
        rc, total = prover.verify_segment(descs, pf, 5, 4, logup, preprocessed=keys)
        want_rc, want_total = prover.verify_segment(descs, pf, 5, 4, logup)
        assert rc == want_rc == 0 and (total == want_total).all()
    rng = np.random.default_rng(5)
    codes = set()
    for pos in list(range(0, 24)) + [int(x) for x in rng.integers(24, len(pf), 40)] + [len(pf) - 1]:
        bad = pf.copy()
        bad[pos] = (int(bad[pos]) + 1 + int(rng.integers(0, 1000))) % P
        want = prover.verify_segment(descs, bad, 5, 4, logup)[0]
        assert want != 0
        assert prover.verify_segment(descs, bad, 5, 4, logup, preprocessed=zero)[0] == want, pos
        codes.add(want)
    assert len(codes) >= 3
    for cut in (pf[:-1], pf[:40], np.concatenate([pf, pf[:1]])):
        assert prover.verify_segment(descs, cut, 5, 4, logup, preprocessed=none)[0] == prover.verify_segment(descs, cut, 5, 4, logup)[0]


def test_a_pws3_proof_against_a_key_with_preprocessed_columns_is_a_header_mismatch(oracle_segment):
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    for a in range(len(airs)):
        keys = [None] * len(airs)
        keys[a] = (2, np.arange(8, dtype=np.uint32))
        assert prover.verify_segment(descs, pf, 5, 4, logup, preprocessed=keys)[0] == 1


def test_operands_past_the_combined_bound_are_malformed(oracle_segment):
    from powdr_amd import prover

    logup, airs, pf = oracle_segment
    descs = descs_of(airs)
    W, lh, bc, sp, it = descs[1]
    # a constraint that names column W (main width W, no preprocessed columns) -> 15
    bad_bc = np.concatenate([np.asarray(bc, np.uint32), np.array([om.OP_PUSH_APC, W], np.uint32)])
    bad_sp = np.asarray(sp, np.uint32).reshape(-1, 2).copy()
    bad_sp[0] = (len(bc), 2)
    bad = list(descs)
    bad[1] = (W, lh, bad_bc, bad_sp, it)
    zero = [None] * len(airs)
    assert prover.verify_segment(bad, pf, 5, 4, logup)[0] == 15
    assert prover.verify_segment(bad, pf, 5, 4, logup, preprocessed=zero)[0] == 15
    # a root word >= p is a malformed key
    keys = [None] * len(airs)
    keys[0] = (1, np.full(8, P, np.uint32))
    assert prover.verify_segment(descs, pf, 5, 4, logup, preprocessed=keys)[0] == 15


def test_fixed_layout_interaction_tables_name_the_preprocessed_operands():
    """The chips' layout: main [multiplicities] | pre [tuple]. The argument operands are the preprocessed columns and the
    multiplicity operands the main ones, and the group structure is the one the main layout has."""
    from powdr_amd import periphery, prover

    for fixed, main, W, Wf in ((periphery.var_range_interactions_pre(), periphery.var_range_interactions(), 1, 2),
                               (periphery.tuple2_interactions_pre(), periphery.tuple2_interactions(), 1, 2),
                               (periphery.bitwise_interactions_pre(), periphery.bitwise_interactions(), 2, 3)):
        it, sp, bc = fixed
        assert (it == main[0]).all()

        def columns(o, n):  # the column operands of one post-fix program
            out, k = [], o
            while k < o + n:
                op = int(bc[k])
                if op in (om.OP_PUSH_APC, om.OP_PUSH_CONST):
                    if op == om.OP_PUSH_APC:
                        out.append(int(bc[k + 1]))
                    k += 2
                else:
                    k += 1
            return out

        for bus, na, first in it:
            assert all(c < W for c in columns(*sp[first]))  # multiplicity: main columns
            args = [c for j in range(1, na + 1) for c in columns(*sp[first + j])]
            assert args and all(W <= c < W + Wf for c in args)  # the tuple: preprocessed columns
        assert max(c for o, n in sp for c in columns(o, n)) == W + Wf - 1
        assert (prover.logup_group_starts(fixed) == prover.logup_group_starts(main)).all()


def test_rust_mirror_has_the_preprocessed_struct():
    from tests.test_rust_adapter_sync import c_struct_fields, rust_struct_fields

    assert c_struct_fields("PwAirPreprocessed") == rust_struct_fields("PwAirPreprocessed") == ["width", "root8"]
