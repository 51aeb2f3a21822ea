"""Edge-valued traces (tests/_edge_values.py) without a GPU:
  a. every case of the table (the one a GPU proof test of these traces iterates) is a valid case: the oracle proves it, and the oracle's verifier and the product's
     host verifier answer what _edge_values.expected_code() says;
  b. the run-time specialised kernels' generated code, executed on the host, with the CHALLENGES at their extremes as well (the
     one place where they can be chosen: on the device the transcript derives them);
  c. the interpreters' host mirrors (the accumulator code of xbc.hpp, the small forms) on rows of every trace kind."""
import ctypes as C

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _edge_values as ev

P = ev.P


def test_word_is_the_value_behind_a_device_word():
    for w in (0, 1, P - 1, (P - 1) // 2, (P + 1) // 2):
        assert int(om.to_monty(np.array([ev.word(w)], np.uint32))[0]) == w
    assert len(set(ev.EDGE.tolist())) == 9 and int(ev.EDGE.max()) < P
    for air in ev.AIRS:
        W, (bc, spans), (inter, ispans, ibc) = ev.air_tables(air)
        assert W == {"hand": 9, "wide": 67, "one": 1}[air]
    # `wide`: the group of three holds the two interactions with identical arguments; every argument count 0 .. 5 occurs
    from powdr_amd import prover

    W, _, it = ev.air_tables("wide")
    assert prover.logup_group_starts(it).tolist()[:2] == [0, 3] and sorted(set(it[0][:, 1].tolist())) == [0, 1, 2, 3, 4, 5]
    assert W % 4 == 3 and W > 64


# ---------------------------------------------------------------------------------------------------------------- a
@pytest.mark.parametrize("air,log_h", ev.CASES)
def test_every_case_is_provable_and_both_verifiers_answer_the_table(air, log_h):
    from powdr_amd import prover

    W, (bc, spans), it = ev.air_tables(air)
    nq, pb = ev.NUM_QUERIES, ev.POW_BITS
    for kind in ev.kinds(air):
        flat = ev.trace(air, kind, log_h)
        assert flat.dtype == np.uint32 and flat.shape == (W << log_h,) and int(flat.max()) < P
        code = ev.expected_code(air, kind, log_h)
        # what the table must say, whatever the evaluator in _edge_values.py found: an AIR without constraints cannot fail the
        # constraint identity; of the others only the kinds declared as satisfying (the satisfied trace, the all-zero trace) pass it
        satisfied = len(spans) == 0 or kind in ev.SATISFYING_KINDS
        assert code == (0 if satisfied else 2), (kind, code)
        pf = sm.prove(flat, W, log_h, bc, spans, num_queries=nq, pow_bits=pb)
        assert sm.verify(pf, W, log_h, bc, spans, num_queries=nq, pow_bits=pb) == code, kind
        assert prover.verify(pf, W, log_h, bc, spans, num_queries=nq, pow_bits=pb) == code, kind
        pf = sm.prove_logup(flat, W, log_h, bc, spans, *it, num_queries=nq, pow_bits=pb)
        assert sm.verify_logup(pf, W, log_h, bc, spans, *it, num_queries=nq, pow_bits=pb) == code, kind
        rc, s = prover.verify_logup(pf, W, log_h, bc, spans, it, num_queries=nq, pow_bits=pb)
        assert rc == code, kind
        if kind == "all_padding" and air == "one":
            assert (s == 0).all()  # no row contributes: the cumulative bus sum is zero


def test_the_kinds_are_what_they_are_called():
    """the properties the kinds exist for, stated on the matrices themselves"""
    half_lo, half_hi = ev.word((P - 1) // 2), ev.word((P + 1) // 2)
    for air in ev.AIRS:
        W = ev.air_tables(air)[0]
        for log_h in (2, 8):
            H = 1 << log_h
            t = lambda kind: ev.trace(air, kind, log_h).reshape(W, H)
            for n, v in zip(ev.EDGE_NAMES, ev.EDGE.tolist()):
                assert (t(f"const[{n}]") == v).all()
            assert all((t("const_by_column")[c] == ev.EDGE[c % 9]).all() for c in range(W))
            assert np.isin(t("cells"), ev.EDGE).all()
            for run in (4, 16):
                m = t(f"runs{run}")
                assert (m == m[0]).all() and all(int(m[0, r]) == (half_lo if (r // run) % 2 == 0 else half_hi) for r in range(H))
            assert not t("spike_first")[:, 1:].any() and not t("spike_last")[:, :-1].any()
            assert np.isin(t("spike_first")[:, 0], ev.EDGE).all() and np.isin(t("spike_last")[:, -1], ev.EDGE).all()
            assert not t("all_padding")[ev.multiplicity_columns(air)].any()
    assert len(np.unique(ev.trace("wide", "cells", 8))) == 9  # every edge value occurs
    c = ev.trace("wide", "cancel", 8).reshape(67, -1)
    assert (c[ev.WIDE_CANCEL[0]] == 1).all() and (c[ev.WIDE_CANCEL[1]] == P - 1).all()
    assert ev.first_violation("hand", ev.trace("hand", "satisfied", 8)) is None
    assert ev.first_violation("hand", ev.trace("hand", "cells", 8)) is not None
    # the vectorised evaluator behind expected_code() against the row-by-row one
    W, (bc, spans), _ = ev.air_tables("wide")
    T = ev.trace("wide", "cells", 4).reshape(W, -1)
    for off, ln in spans.tolist():
        assert ev.eval_postfix_columns(bc[off:off + ln].tolist(), T).tolist() == [ev.eval_postfix(bc[off:off + ln], T[:, r]) for r in range(T.shape[1])]


# ---------------------------------------------------------------------------------------------------------------- b
N_ROWS = 24


def _challenge_tables(n_apow):
    """{name: (al[4], blpow[9, 4], apow[n_apow, 4])}, canonical: every coordinate's DEVICE word is one of CHALLENGE_WORDS"""
    n = 4 + 36 + 4 * n_apow
    out = {}
    for name, w in (("all (p-1)/2", (P - 1) // 2), ("all (p+1)/2", (P + 1) // 2), ("all p-1", P - 1), ("all 1", 1)):
        out[name] = np.full(n, ev.word(w), np.int64)
    words = np.array([ev.word(w) for w in ev.CHALLENGE_WORDS], np.int64)
    for seed in (1, 2):
        out[f"drawn {seed}"] = words[np.random.default_rng(seed).integers(0, 4, n)]
    return {k: (v[:4], v[4:40].reshape(9, 4), v[40:].reshape(n_apow, 4)) for k, v in out.items()}


@pytest.mark.parametrize("air,chunk_costs", [("hand", (200, 100000)), ("wide", (200, 100000))])
def test_generated_code_on_the_host_with_edge_traces_and_extreme_challenges(tmp_path, air, chunk_costs):
    """test_jit.py::test_generated_code_runs_on_the_host_and_means_what_it_should on edge data: T and the committed permutation
    columns Pm from the trace kinds, alpha / the powers of beta / the constraint challenge's powers with every coordinate's device word
    in {(p-1)/2, (p+1)/2, p-1, 1} (among them the tables that are (p-1)/2 and (p+1)/2 throughout: every centred term of an accumulator
    at its extreme, with one sign), for a split into several chunks and units and for one chunk. Same assertions: the permutation
    columns, the row sums and the quotient parts equal the values computed with plain integers."""
    from powdr_amd import prover
    from tests._jit_host import GeneratedCodeOnTheHost, ext_inv_tower, expected_values

    W, (bc, spans), it = ev.air_tables(air)
    starts = prover.logup_group_starts(it)
    n_groups, n_cons = len(starts) - 1, len(spans)
    codes = []
    for cost in chunk_costs:
        sub = tmp_path / str(cost)
        sub.mkdir()
        codes.append(GeneratedCodeOnTheHost(sub, W, bc, spans, it, cost))
        for which in (1, 0):
            units, total = codes[-1].units[which], codes[-1].total[which]
            assert units and total >= (2 if cost == chunk_costs[0] else 1) and sum(u["n_chunks"] for u in units) == total
    # several chunks, and as few as the generator makes: one for the permutation columns, constraints and LogUp terms apart in the quotient
    assert all(codes[0].total[w] > codes[1].total[w] for w in (1, 0)) and codes[1].total[1] == 1 and codes[1].total[0] <= 2
    for cname, (al, blpow, apow) in _challenge_tables(n_cons + n_groups + 2).items():
        for k, kind in enumerate(ev.kinds(air)):
            pm_kind = kind if kind in ev.TRACE_KINDS else "cells"
            canon = {"T": ev.matrix(kind, W, N_ROWS, 7 + k, air).astype(np.int64), "Pm": ev.matrix(pm_kind, 4 * n_groups + 4, N_ROWS, 70 + k).astype(np.int64),
                     "apow": apow, "al": al, "blpow": blpow}
            q_want, quot_want = expected_values(bc, spans, it, starts, canon, N_ROWS, ext_inv=ext_inv_tower)
            for code, cost in zip(codes, chunk_costs):
                code.check(canon, N_ROWS, q_want, quot_want, what=f"{air}, chunk cost {cost}, challenges {cname}, trace {kind}")


# ---------------------------------------------------------------------------------------------------------------- c
@pytest.mark.parametrize("air", ["hand", "wide"])
def test_interpreter_host_mirrors_on_edge_rows(air):
    """powdr_xbc_eval_host (the accumulator code the interpreter kernels run) and powdr_small_form_eval_host (the closed forms of the
    fast bus kernels) against the post-fix evaluator in plain integers: every span of the AIR — constraints, multiplicities, arguments
    — on the distinct rows of every trace kind."""
    from powdr_amd import abi

    lib = abi.lib
    lib.powdr_xbc_eval_host.restype = C.c_int
    lib.powdr_small_form_eval_host.restype = C.c_int
    W, (bc, spans), (inter, ispans, ibc) = ev.air_tables(air)
    programs = [np.ascontiguousarray(bc[o:o + n]) for o, n in spans.tolist()] + [np.ascontiguousarray(ibc[o:o + n]) for o, n in ispans.tolist()]
    rows = np.unique(np.concatenate([ev.trace(air, kind, 5).reshape(W, -1).T for kind in ev.kinds(air)]), axis=0)
    assert len(rows) > 100
    rows_m = om.to_monty(np.ascontiguousarray(rows, np.uint32))
    small = 0
    for prog in programs:
        for row, row_m in zip(rows, rows_m):
            want = ev.eval_postfix(prog, row)
            res, aux = C.c_uint32(), C.c_uint32()
            args = (prog.ctypes.data_as(C.c_void_p), C.c_uint32(len(prog)), row_m.ctypes.data_as(C.c_void_p), C.c_size_t(0), C.byref(res), C.byref(aux))
            assert lib.powdr_xbc_eval_host(*args) == 0  # (column operand c of a one-row matrix: trace[c + 0])
            assert int(om.from_monty(np.array([res.value], np.uint32))[0]) == want, (prog.tolist(), row.tolist())
            rc = lib.powdr_small_form_eval_host(*args)
            assert rc in (0, 1)
            if rc == 0:  # (1: no small form, the interpreter's case)
                small += 1
                assert int(om.from_monty(np.array([res.value], np.uint32))[0]) == want, (prog.tolist(), row.tolist())
    assert small >= len(rows) * len(ispans) // 2  # most multiplicities and arguments are small forms
