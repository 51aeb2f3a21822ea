"""pw-stark v1 + public values, the host side: what the prover entry and the host verifier accept as an AIR with public
values, the PWS5 / PWS6 headers against descriptions with and without them, the public connector's constraints on a numpy model, the
links of a chain, and the Rust declarations. No GPU: the prover-side checks go through the host-only creation path."""
import numpy as np
import pytest

from oracle import apc_model as om
from tests.test_preprocessed_segment_gpu import NO_INTER, cons_tables, tables

P = om.P
PA, PC, ADD, SUB, MUL, NEG = 0, 1, 2, 3, 4, 5
MAGIC5, MAGIC6 = 0x35535750, 0x36535750
W, WF, NP = 3, 1, 2  # main columns, preprocessed columns, public values of the AIR the checks are made on: W1 = 4


def rows():
    from powdr_amd.prover import row_operands

    return row_operands(W, WF)


def power(pv, c, k):
    """pv * c^k as a post-fix program"""
    code = [PA, pv]
    for _ in range(k):
        code += [PA, c, MUL]
    return code


def cases():
    """(name, constraints, interactions, n_public, accepted)"""
    r = rows()
    ok = [PA, 0, PA, r.public(1), SUB]
    bad_inter = tables([(5, [PA, 0], [[PA, W + WF]])])  # an interaction operand at W1: the next row of column 0
    pub_inter = tables([(5, [PA, 0], [[PA, r.public(0)]])])
    good_inter = tables([(5, [PA, W], [[PA, 0]])])  # the preprocessed column: below W1
    return [("a public operand", [ok], None, NP, True),
            ("the last public operand", [[PA, r.public(NP - 1)]], None, NP, True),
            ("the operand behind the public values", [[PA, r.bound + NP]], None, NP, False),
            ("a public operand of an AIR without", [[PA, r.public(0)]], None, 0, False),
            ("256 public values", [[PA, r.public(255), PA, 1, SUB]], None, 256, True),
            ("257 public values", [ok], None, 257, False),
            ("an interaction operand at W1", [ok], bad_inter, NP, False),
            ("a public operand in an interaction", [ok], pub_inter, NP, False),
            ("interactions below W1", [ok], good_inter, NP, True),
            ("pv c^3", [power(r.public(0), 1, 3)], None, NP, True),
            ("pv c^4", [power(r.public(0), 1, 4)], None, NP, False),
            ("pv is_transition c^3", [power(r.public(0), 1, 3) + [PA, r.is_transition, MUL]], None, NP, True),
            ("an unbalanced program", [[PA, r.public(0), MUL]], None, NP, False)]


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_prover_entry_checks(case):
    from powdr_amd import prover

    _, progs, inter, n_public, accepted = case
    got = prover.public_programs_check(W, *cons_tables(progs), n_public, interactions=inter, pre_width=WF)
    assert (got is not None) == accepted


def test_degree_flags_and_code_of_accepted_airs():
    from powdr_amd import prover

    r = rows()
    got = prover.public_programs_check(W, *cons_tables([power(r.public(0), 1, 3)]), NP, pre_width=WF)
    assert got["max_degree"] == 3 and got["row_flags"] == 0  # a public value has degree 0; public values alone make no AIR row-aware
    got = prover.public_programs_check(W, *cons_tables([[PA, r.is_first_row, PA, 0, PA, r.public(0), SUB, MUL],
                                                        [PA, r.next(1), PA, r.public(1), MUL]]), NP, pre_width=WF)
    assert got["max_degree"] == 2 and got["row_flags"] == 3
    # xbc: public leaves are the *_PUB forms (17 .. 22) with the INDEX as operand, never folded; the generated kernels read pub[index]
    ops, operands = got["xbc"][0::2], got["xbc"][1::2]
    assert sorted(int(a) for o, a in zip(ops, operands) if o >= 17) == [0, 1] and (ops <= 22).all()
    assert "const uint32_t* __restrict__ pub)" in got["source"] and "pub[0u]" in got["source"] and "pub[1u]" in got["source"]
    # constants fold, public values do not: (2 + 3) * pv1 is SET_CONST 5, MUL_PUB 1
    got = prover.public_programs_check(W, *cons_tables([[PC, 2, PC, 3, ADD, PA, r.public(1), MUL]]), NP, pre_width=WF)
    assert got["xbc"].reshape(-1, 2)[:, 0].tolist() == [1, 22] and int(om.from_monty(got["xbc"][1:2])[0]) == 5 and got["xbc"][3] == 1


def test_an_air_without_public_values_compiles_to_the_code_of_the_existing_entries():
    """n_public = 0: the generated source of the quotient kernels (a function of the xbc code) is the text the existing test hook
    gives for the same programs — no argument, no read, no form is added for an AIR that has no public values."""
    from powdr_amd import prover
    from tests.test_segment_proof import SPEC, synthetic_airs

    for a in synthetic_airs(SPEC):
        for inter in (None, a[5]):
            new = prover.public_programs_check(a[1], a[3], a[4], 0, interactions=inter)
            old, _ = prover.jit_generated_sources(a[1], a[3], a[4], interactions=inter, which=0)
            assert new["source"] == "".join(u["source"] for u in old) and "pub" not in new["source"]
            assert (new["xbc"][0::2] <= 16).all()


def _desc(progs, inter):
    return (W, 3, *cons_tables(progs), inter)


@pytest.mark.parametrize("case", cases(), ids=[c[0] for c in cases()])
def test_verifier_description_checks(case):
    """the verifier holds an AIR with public values to what its prover entry checks: 15 before it looks at the proof"""
    from powdr_amd import prover

    _, progs, inter, n_public, accepted = case
    logup = inter is not None
    hdr = np.array([MAGIC6, 1, int(logup), 4, 0, 3, W, len(progs), len(inter[0]) if logup else 0], np.uint32)
    pf = np.concatenate([hdr, np.zeros(400, np.uint32)])
    key = [(WF, np.zeros(8, np.uint32))]
    rc = prover.verify_segment([_desc(progs, inter)], pf, 4, 0, logup, preprocessed=key, public=[n_public or None])[0]
    if n_public == 0:
        assert rc == 15  # (the operand is past the row layout of an AIR without public values)
    else:
        assert (rc == 15) == (not accepted) and (accepted is False or rc not in (1, 15))


def test_headers():
    from powdr_amd import prover

    r = rows()
    with_pub, without = _desc([[PA, 0, PA, r.public(0), SUB]], None), _desc([[PA, 0, PA, 1, SUB]], None)
    key = [(WF, np.zeros(8, np.uint32))]

    def proof(magic):
        return np.concatenate([np.array([magic, 1, 0, 4, 0, 3, W, 1, 0], np.uint32), np.zeros(400, np.uint32)])

    # a PWS5 proof against descriptions with public values, a PWS6 proof against descriptions without: not their header
    assert prover.verify_segment([with_pub], proof(MAGIC5), 4, 0, False, preprocessed=key, public=[NP])[0] == 1
    assert prover.verify_segment([without], proof(MAGIC6), 4, 0, False, preprocessed=key, public=[None])[0] == 1
    assert prover.verify_segment([without], proof(MAGIC6), 4, 0, False, preprocessed=key, transition=True)[0] == 1
    # the matching header gets past that check (and fails later: the rest is zeros)
    assert prover.verify_segment([with_pub], proof(MAGIC6), 4, 0, False, preprocessed=key, public=[NP])[0] not in (0, 1, 15)
    # the values a proof carries are read by the description's count; a header that does not match: refused
    pf = proof(MAGIC6)
    pf[9:11] = (41, 42)
    assert prover.segment_public_values([with_pub], pf, [NP], 0).tolist() == [41, 42]
    assert prover.verify_segment([with_pub], pf, 4, 0, False, preprocessed=key, public=[[41, 43]])[0] == 17
    assert prover.verify_segment([with_pub], pf, 4, 0, False, preprocessed=key, public=[[41, 42]])[0] not in (0, 1, 15, 17)
    for bad in (proof(MAGIC5), pf[:10]):
        with pytest.raises(ValueError):
            prover.segment_public_values([with_pub], bad, [NP], 0)
    with pytest.raises(ValueError):
        prover.segment_public_values([without], pf, [None], 0)


# ---- the public connector -------------------------------------------------------------------------------------------------------------
def evaluate(code, operand):
    """a post-fix program over Python integers mod p; operand(c) = the value of column operand c"""
    st = []
    it = iter(code)
    for op in it:
        if op == PA:
            st.append(operand(int(next(it))) % P)
        elif op == PC:
            st.append(int(next(it)) % P)
        elif op == NEG:
            st.append(-st.pop() % P)
        else:
            b, a = st.pop(), st.pop()
            st.append((a + b if op == ADD else a - b if op == SUB else a * b) % P)
    assert len(st) == 1
    return st[0]


def connector_violations(trace, public):
    """[(row, constraint)] of the public connector on a 2 x 2 main trace [pc, timestamp] with its fixed column is_end = (0, 1)"""
    from powdr_amd import system_airs as sa

    air = sa.connector_air(public=True)
    bc, spans = air.cons
    r = rows_of_connector()
    out = []
    for row in range(2):
        vals = {0: trace[0][row], 1: trace[1][row], 2: int(air.fixed[0][row])}
        vals.update({r.public(k): public[k] for k in range(4)})
        for c, (off, ln) in enumerate(spans):
            if evaluate(bc[off:off + ln].tolist(), lambda a: vals[a]):
                out.append((row, c))
    return out


def rows_of_connector():
    from powdr_amd.prover import row_operands

    return row_operands(2, 1)


def test_public_connector_model():
    from powdr_amd import prover, system_airs as sa

    air = sa.connector_air(public=True)
    assert sa.CONNECTOR_PUBLIC == ["start_pc", "start_ts", "end_pc", "end_ts"] and air.n_public == 4 and len(air.cons[1]) == 4
    assert (air.width, air.pre_width, air.log_h, air.columns) == (2, 1, 1, ["pc", "timestamp"]) and len(air.inter[0]) == 1
    plain = sa.connector_air()
    assert plain.n_public == 0 and len(plain.cons[1]) == 0 and all((x == y).all() for x, y in zip(plain.inter, air.inter))
    got = prover.public_programs_check(2, *air.cons, 4, interactions=air.inter, pre_width=1)
    assert got["max_degree"] == 2 and got["row_flags"] == 0  # public-only: no next row, no selector
    start, end = (0x200000, 1), (0x200040, 97)
    trace, public = [[start[0], end[0]], [start[1], end[1]]], [*start, *end]
    assert connector_violations(trace, public) == []
    # each value changed by one: exactly its constraint, on its row
    for k in range(4):
        bad = list(public)
        bad[k] = (bad[k] + 1) % P
        assert connector_violations(trace, bad) == [(k // 2, k)]
    # and a trace whose rows are swapped satisfies none of the four
    assert connector_violations([[end[0], start[0]], [end[1], start[1]]], public) == [(0, 0), (0, 1), (1, 2), (1, 3)]


def test_connector_links():
    from powdr_amd import system_airs as sa

    k = sa.CONNECTOR_PUBLIC.index
    assert sa.connector_links(7) == [(7, k("end_pc"), 7, k("start_pc")), (7, k("end_ts"), 7, k("start_ts"))] == [(7, 2, 7, 0), (7, 3, 7, 1)]


def test_chain_of_unverifiable_segments_names_the_first():
    """the chain verifier returns the segment verifier's code and the index of the first failing segment (host only)"""
    from powdr_amd import prover

    r = rows()
    d = _desc([[PA, 0, PA, r.public(0), SUB]], None)
    pf = np.concatenate([np.array([MAGIC6, 1, 0, 4, 0, 3, W, 1, 0], np.uint32), np.zeros(400, np.uint32)])
    seg = dict(descs=[d], proof=pf, public=[NP], preprocessed=[(WF, np.zeros(8, np.uint32))])
    want = prover.verify_segment([d], pf, 4, 0, False, preprocessed=seg["preprocessed"], public=[NP])[0]
    assert want != 0 and prover.verify_segment_chain([seg, seg], [(0, 0, 0, 1)], 4, 0) == (want, 0)


def test_rust_binds_the_public_value_entries():
    import re

    from tests.test_rust_adapter_sync import FFI, c_functions, c_struct_fields, rust_functions

    c, r = c_functions(), rust_functions()
    for name in ("pw_prover_create_public", "pw_prover_n_public", "pw_prover_set_public_values", "pw_verify_segment_public",
                 "pw_segment_proof_public_values", "pw_verify_segment_chain"):
        assert name in c and r.get(name) == c[name]
    for name in ("PwAirPublic", "PwChainSegment", "PwChainLink"):
        rust = re.findall(r"pub (\w+)\s*:", re.search(r"pub struct " + name + r"\s*\{([^}]*)\}", FFI, flags=re.S).group(1))
        assert [f.rstrip("_") for f in rust] == c_struct_fields(name)  # (`pub` is a Rust keyword: the field is `pub_`)
