"""Random AIRs (tests/_random_airs.py) on the CPU: the census of what the GPU tests' seed lists contain, the generated code of the run-time
specialised kernels executed on the host against plain modular arithmetic, the two host verifiers on the oracle's proofs, and the
malformed programs neither the product nor the oracle may evaluate. The device half is test_random_airs_gpu.py."""
import collections
import functools

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _random_airs as ra
from tests._edge_values import _programs

P = ra.P
PA, PC, ADD, SUB, MUL, NEG = ra.PA, ra.PC, ra.ADD, ra.SUB, ra.MUL, ra.NEG
NQ, PB = 4, 0

# ---- the seed lists of test_random_airs_gpu.py (it imports them from here: the census below is about exactly these) ------------------
PROOF_SEEDS = list(range(24))
PINNED_HEIGHTS = {7: 12, 9: 12, 12: 13}  # two seeds on the fused LDE schedule; one whose LogUp prefix scan crosses its 4096-row block
JIT_SEEDS = [1, 3, 4, 8, 12, 13, 14, 18]
SEGMENT_SEEDS = [0, 5, 10, 15, 20, 23]
MOCK_SEEDS = [3, 4, 6, 8, 9, 12, 14, 15, 18, 19, 22, 23]
ROW_AWARE_SEEDS = [0, 1, 2, 3, 4, 5]
HOST_CODE_SEEDS = [0, 2, 3, 4, 5, 8, 12, 13, 15, 16, 17, 19]
HOST_CODE_SEEDS_SLOW = [1, 6, 7, 9, 10, 11, 14, 18]


def proof_log_height(seed: int) -> int:
    """2^1 .. 2^6 rows, every height several times over PROOF_SEEDS; the pinned seeds 2^12 / 2^13"""
    return PINNED_HEIGHTS.get(seed, 1 + (5 * seed + 2) % 6)


def proof_trace_kind(seed: int) -> str:
    return ra.TRACE_KINDS[seed % 4]


def segment_airs(seed: int):
    """three random AIRs of different heights (2^2 .. 2^7): [(flat trace, W, log_h, bc, spans, it)]"""
    rng = np.random.default_rng([0x534547, seed])
    heights = rng.choice(np.arange(2, 8), 3, replace=False).tolist()
    out = []
    for k, log_h in enumerate(heights):
        W, (bc, spans), it, meta = ra.random_air(3 * seed + k)
        out.append((ra.trace(meta, log_h, ra.TRACE_KINDS[(seed + k) % 4]), W, log_h, bc, spans, it if len(it[0]) else None))
    return out


MOCK_LOG_HEIGHT = 5


@functools.lru_cache(maxsize=None)
def _air(seed):
    return ra.random_air(seed)


# ---------------------------------------------------------------------------------------------------------------- census
def test_census_of_the_seed_lists():
    """Conditions on the INPUTS of the GPU tests: over the committed seed lists every planted shape and every property the generator
    promises occurs at least twice, no seed is skipped, and the generator's own book-keeping (degrees, groups) is what the product and
    the oracle compute from the programs."""
    from powdr_amd import prover

    plants, props = collections.Counter(), collections.Counter()
    for seed in PROOF_SEEDS:
        W, (bc, spans), it, meta = _air(seed)
        assert meta["W"] == W and 1 <= W <= 70
        chk = prover.public_programs_check(W, bc, spans, 0, it if len(it[0]) else None)
        assert chk is not None, seed
        assert chk["max_degree"] == meta["max_degree"] == max(meta["constraint_degrees"], default=0), seed
        assert len(spans) == len(meta["constraints"]) and len(it[0]) == len(meta["interactions"])
        assert ("no_constraints" in meta["plants"]) == (len(spans) == 0) and ("no_interactions" in meta["plants"]) == (len(it[0]) == 0)
        sizes = []
        if len(it[0]):
            starts = prover.logup_group_starts(it)
            assert (starts == sm.group_starts(*it)).all(), seed
            sizes = ra.group_sizes(starts)
            assert sum(sizes) == len(it[0])
        for p in meta["plants"]:
            plants[p] += 1
        props[f"W%4={W % 4}"] += 1
        props["W>64"] += W > 64
        props["W==64"] += W == 64
        props["W==1"] += W == 1
        props["group>=3"] += any(s >= 3 for s in sizes)
        props["group==1"] += any(s == 1 for s in sizes)
        props["depth16"] += meta["max_stack_depth"] == 16
        props["depth15"] += meta["max_stack_depth"] == 15
        for n in set(meta["n_args"]):
            props[f"n_args={n}"] += 1
        for d in set(meta["constraint_degrees"]):
            props[f"constraint_degree={d}"] += 1
        for d in set(meta["multiplicity_degrees"]):
            props[f"multiplicity_degree={d}"] += 1
        for d in set(meta["argument_degrees"]):
            props[f"argument_degree={d}"] += 1
        props[f"trace={proof_trace_kind(seed)}"] += 1
        props[f"log_h={proof_log_height(seed)}"] += 1
        props["homogeneous"] += meta["homogeneous"]
    want = ([f"W%4={k}" for k in range(4)] + ["W>64", "W==1", "group>=3", "group==1", "depth16", "depth15", "homogeneous"] +
            [f"n_args={n}" for n in range(8)] + [f"constraint_degree={d}" for d in (1, 2, 3)] + [f"multiplicity_degree={d}" for d in (0, 1, 2, 3)] +
            [f"argument_degree={d}" for d in (0, 1, 2)] + [f"trace={k}" for k in ra.TRACE_KINDS] + [f"log_h={h}" for h in range(1, 7)])
    assert all(plants[p] >= 2 for p in ra.PLANTS), {p: plants[p] for p in ra.PLANTS}
    assert all(props[k] >= 2 for k in want), {k: props[k] for k in want if props[k] < 2}
    assert props["W==64"] >= 1 and props["log_h=12"] == 2 and props["log_h=13"] == 1
    # the specialised-kernel seeds hold the depth-16 chains of all three kinds and a group of three or more
    jit_plants = set().union(*[_air(s)[3]["plants"] for s in JIT_SEEDS])
    assert {"chain16_constraint", "chain16_multiplicity", "chain16_argument"} <= jit_plants
    assert any(max(ra.group_sizes(prover.logup_group_starts(_air(s)[2]))) >= 3 for s in JIT_SEEDS)
    assert set(JIT_SEEDS) <= set(PROOF_SEEDS) and len(JIT_SEEDS) == 8 and len(PROOF_SEEDS) == 24 and len(SEGMENT_SEEDS) == 6
    assert len(MOCK_SEEDS) == 12 and len(ROW_AWARE_SEEDS) == 6 and len(HOST_CODE_SEEDS) >= 12
    # segments: three different heights between 2^2 and 2^7, AIRs with and without interactions
    for seed in SEGMENT_SEEDS:
        hs = [a[2] for a in segment_airs(seed)]
        assert len(set(hs)) == 3 and all(2 <= h <= 7 for h in hs)
    assert sum(any(a[5] is None for a in segment_airs(s)) for s in SEGMENT_SEEDS) >= 1


def test_census_of_the_mock_prover_inputs():
    """the zero-rows traces the mock prover is asked about hold clean AND violating rows (several seeds each: both in one trace)"""
    both = 0
    for seed in MOCK_SEEDS:
        meta = _air(seed)[3]
        H = 1 << MOCK_LOG_HEIGHT
        pairs, rows, first = ra.violations(meta["constraints"], ra.trace_matrix(meta, MOCK_LOG_HEIGHT, "zero_rows"))
        assert pairs >= rows and (first is None) == (rows == 0)
        both += 0 < rows < H
    assert both >= 6, both
    assert sum(len(_air(s)[3]["constraints"]) == 0 for s in MOCK_SEEDS) >= 1  # (and an AIR nothing can violate)


@pytest.mark.parametrize("row_aware", [False, True])
def test_derived_airs_are_satisfied_and_balanced(row_aware):
    """derived_air under the generator's own evaluation: no violation, an empty bus; a changed derived cell is a violation at that row
    (and, for a next-row read, the row before); the programs are what the product's creation accepts, of degree <= 3"""
    from powdr_amd import prover

    kinds = collections.Counter()
    for seed in range(12):
        for log_h in (2, 5):
            d = ra.derived_air(seed, log_h, row_aware)
            assert d["check"](d["T"]) == (0, 0, None), (seed, log_h)
            assert ra.bus_tally(d["interactions"], d["T"]) == {}, (seed, log_h)
            chk = prover.public_programs_check(d["W"], *d["cons"], 0 if d["public"] is None else len(d["public"]), d["it"], d["pre_width"])
            assert chk is not None and chk["max_degree"] <= 3, (seed, log_h)
            assert (chk["row_flags"] != 0) == row_aware
            for kind, _ in d["kinds"]:
                kinds[kind] += 1
            bad = d["T"].copy()
            kind, j = d["kinds"][0]
            bad[j, 1] = (int(bad[j, 1]) + 1) % P
            pairs, rows, first = d["check"](bad)
            assert rows >= 1 and first is not None and first[0] in (0, 1), (seed, log_h, first)
            if row_aware:
                wrong = d["public"].copy()
                wrong[0] = (int(wrong[0]) + 1) % P
                assert d["check"](d["T"], wrong)[2] == (0, len(d["constraints"]) - 2)  # is_first_row * (col_0 - pub_0)
    if row_aware:
        assert all(kinds[k] >= 2 for k in ("row", "next", "fixed", "first", "last")), kinds


# ---------------------------------------------------------------------------------------------------------------- generated code
def _host_code_params():
    return [pytest.param(s, id=str(s)) for s in HOST_CODE_SEEDS] + [pytest.param(s, id=str(s), marks=pytest.mark.slow) for s in HOST_CODE_SEEDS_SLOW]


HOST_ROWS = 5  # (expected_values is plain Python: an extension-field inverse per interaction and row)


def _host_inputs(seed):
    """the trace rows: uniform | zero-multiplicity block | zero rows, so that rows where every multiplicity vanishes are among them"""
    meta = _air(seed)[3]
    return np.concatenate([ra.trace_matrix(meta, 0, "uniform", 2), ra.trace_matrix(meta, 0, "zero_multiplicity_block", 2)[:, :1],
                           ra.trace_matrix(meta, 0, "zero_rows", 2)], axis=1).astype(np.int64)


def test_census_of_the_host_code_inputs():
    seeds = HOST_CODE_SEEDS
    assert sum(len(ra.vanishing_multiplicity_rows(_air(s)[3], _host_inputs(s))) >= 1 and len(_air(s)[3]["interactions"]) >= 1 for s in seeds) >= 2
    assert sum(_air(s)[3]["max_stack_depth"] == 16 for s in seeds) >= 2 and sum("no_constraints" in _air(s)[3]["plants"] for s in seeds) >= 2
    assert sum("no_interactions" in _air(s)[3]["plants"] for s in seeds) >= 1
    assert all(_host_inputs(s).shape == (_air(s)[0], HOST_ROWS) for s in seeds)


@pytest.mark.parametrize("seed", _host_code_params())
def test_generated_code_of_random_airs_on_the_host(tmp_path, seed):
    """The specialised kernels' generated code of a random AIR EXECUTED on the host (tests/_jit_host.py), at a chunk cost that cuts both
    kernel families into several chunks and units (a boundary inside a LogUp group or between two constraints) and as one chunk: the
    permutation columns, the per-chunk row sums and the quotient numerator's parts equal plain modular arithmetic in F_p^4."""
    from powdr_amd import prover

    from tests._jit_host import GeneratedCodeOnTheHost, expected_values, ext_inv_tower

    W, (bc, spans), it, meta = _air(seed)
    has_it = len(it[0]) > 0
    starts = prover.logup_group_starts(it) if has_it else np.zeros(1, np.uint32)
    n_groups, n_cons, N = len(starts) - 1, len(spans), HOST_ROWS
    rng = np.random.default_rng([0x484f5354, seed])
    canon = {"T": _host_inputs(seed), "Pm": rng.integers(0, P, (4 * n_groups + 4, N)), "apow": rng.integers(0, P, (n_cons + n_groups + 2, 4)),
             "al": rng.integers(0, P, 4), "blpow": rng.integers(0, P, (9, 4))}
    q_want, quot_want = expected_values(bc, spans, it, starts, canon, N, ext_inv=ext_inv_tower)
    for chunk_cost in (60, 10 ** 6):
        code = GeneratedCodeOnTheHost(tmp_path, W, bc, spans, it if has_it else None, chunk_cost)
        for which in (1, 0):
            units, total = code.units[which], code.total[which]
            if which == 1 and not has_it:
                assert not units
                continue
            assert units and sum(u["n_chunks"] for u in units) == total
            if chunk_cost == 60 and (n_cons + n_groups >= 2 if which == 0 else n_groups >= 2):
                assert total >= 2, (seed, which, total)
            if chunk_cost != 60:  # (the quotient keeps its constraints and its LogUp terms apart: two chunks at the most)
                assert total <= (2 if which == 0 else 1), (seed, which, total)
        code.check(canon, N, q_want, quot_want, f"seed {seed}, chunk cost {chunk_cost}")


def test_the_small_chunk_cost_cuts_both_families_of_most_host_code_seeds():
    """(the `total >= 2` of the test above is conditional on there being two things to separate: here, that it mostly is)"""
    from powdr_amd import prover

    n = collections.Counter()
    for seed in HOST_CODE_SEEDS:
        W, (bc, spans), it, meta = _air(seed)
        for which in (1, 0):
            n[which] += prover.jit_generated_sources(W, bc, spans, it if len(it[0]) else None, which, 60, 2)[1] >= 2
    assert n[0] >= 8 and n[1] >= 6, n


# ---------------------------------------------------------------------------------------------------------------- verifiers
def _flip(pf, rng):
    out = pf.copy()
    i = int(rng.integers(0, len(out)))
    out[i] = (int(out[i]) + 1) % P
    return out


def test_both_host_verifiers_agree_on_the_oracles_proofs():
    """prover.verify* and sm.verify* on the oracle's proofs of 100 random AIRs and 12 derived (satisfied) ones, 2^1 .. 2^6 rows,
    constraints only and with LogUp: the same code; the code is 0 exactly where the generator's evaluation finds no violation; one
    changed word is rejected by both with the same code."""
    from powdr_amd import prover

    codes = collections.Counter()
    cases = [(ra.random_air(s)[:3], None, s) for s in range(100)]
    for s in range(12):
        d = ra.derived_air(s, 1 + s % 6)
        cases.append(((d["W"], d["cons"], d["it"]), d, s))
    for (W, (bc, spans), it), d, seed in cases:
        rng = np.random.default_rng([0x564552, seed])
        if d is None:
            meta = _air(seed)[3]
            log_h = 1 + seed % 6
            T = ra.trace_matrix(meta, log_h, ra.TRACE_KINDS[(seed // 6) % 4])
            clean = ra.violations(meta["constraints"], T)[1] == 0
        else:
            log_h, T, clean = d["log_h"], d["T"], True
        flat = T.reshape(-1)
        pf = sm.prove(flat, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)
        a, b = prover.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB), sm.verify(pf, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)
        assert a == b == (0 if clean else 2), (seed, a, b, clean)
        codes[a] += 1
        bad = _flip(pf, rng)
        a, b = prover.verify(bad, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB), sm.verify(bad, W, log_h, bc, spans, num_queries=NQ, pow_bits=PB)
        assert a == b != 0, (seed, a, b)
        if len(it[0]):
            pf = sm.prove_logup(flat, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB)
            a = prover.verify_logup(pf, W, log_h, bc, spans, it, num_queries=NQ, pow_bits=PB)[0]
            b = sm.verify_logup(pf, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB)
            assert a == b == (0 if clean else 2), (seed, a, b, clean)
            codes[a] += 1
            bad = _flip(pf, rng)
            a = prover.verify_logup(bad, W, log_h, bc, spans, it, num_queries=NQ, pow_bits=PB)[0]
            b = sm.verify_logup(bad, W, log_h, bc, spans, *it, num_queries=NQ, pow_bits=PB)
            assert a == b != 0, (seed, a, b)
    assert codes[0] >= 20 and codes[2] >= 20, codes


# ---------------------------------------------------------------------------------------------------------------- malformed programs
MW = 20  # the width of the AIR the malformed programs are planted in


def _chain_words(n, W=MW):
    return [w for c in range(n) for w in (PA, c % W)] + [ADD] * (n - 1)


MALFORMED = {
    "depth17": _chain_words(17),
    "depth40": _chain_words(40),
    "underflow": [PA, 0, ADD],
    "underflow_neg": [NEG],
    "unknown_opcode": [PA, 0, PA, 1, 9],
    "push_without_operand": [PA, 0, PA, 1, ADD, PC],
    "column_W": [PA, MW],
    "column_past_the_row_layout": [PA, 2 * MW + 3],
    "two_values_left": [PA, 0, PA, 1],
    "empty": [],
    "inv_or_zero": [PA, 0, om.OP_INV_OR_ZERO],
}
SPAN_KINDS = ["constraint", "multiplicity", "argument"]


def _planted(kind, words):
    """the AIR with `words` as its second constraint / the multiplicity / the last argument of its second interaction; spans before
    and behind the planted one, so that a PUSH without its operand would read the next span's first word"""
    cons = [[PA, 0, PA, 1, MUL, PA, 2, SUB], words if kind == "constraint" else [PA, 3, PA, 3, MUL], [PA, 4]]
    inter = [(4, [PA, 5], [[PA, 6]]),
             (4, words if kind == "multiplicity" else [PA, 7], [[PA, 8], words if kind == "argument" else [PA, 9]]),
             (4, [PC, 1], [[PA, 10], [PA, 11]])]
    return _programs(cons, inter)


@functools.lru_cache(maxsize=None)
def _well_formed_proofs():
    """the oracle's proofs of the well-formed sibling (same width, same numbers of constraints and interactions: the header a verifier
    of a planted AIR expects)"""
    (bc, spans), it = _planted("constraint", [PA, 3])
    T = np.random.default_rng(5).integers(0, P, (MW, 4)).astype(np.int64)
    T[3], T[4], T[2] = 0, 0, T[0] * T[1] % P  # (satisfied: a segment verifier that meets the sibling first goes on to the planted AIR)
    flat = T.astype(np.uint32).reshape(-1)
    return (sm.prove(flat, MW, 2, bc, spans, num_queries=NQ, pow_bits=PB), sm.prove_logup(flat, MW, 2, bc, spans, *it, num_queries=NQ, pow_bits=PB),
            sm.prove_segment([(flat, MW, 2, bc, spans, it)] * 2, num_queries=NQ, pow_bits=PB, logup=True),
            sm.prove_segment([(flat, MW, 2, bc, spans, it)] * 2, num_queries=NQ, pow_bits=PB, logup=False), flat)


@pytest.mark.parametrize("what", sorted(MALFORMED))
@pytest.mark.parametrize("kind", SPAN_KINDS)
def test_malformed_programs_are_refused_by_the_product_and_by_the_oracle(kind, what):
    """A program that is too deep for the 16-entry evaluation stack (17, 40), underflows it, leaves two values on it, holds an unknown
    opcode or INV_OR_ZERO, a PUSH without its operand or a column the trace does not have - as a constraint, a multiplicity, an
    argument, and in an AIR of a segment: the product makes no prover of it (public_programs_check, jit_generated_sources) and its
    verifiers answer 10 (a segment: 15, a malformed description); the oracle raises from its provers, its verifiers answer the same
    codes, and the interpreter is alive afterwards (before the oracle validated its programs, its verifiers ended the process at
    depth 17 and its provers wrote past their stack)."""
    from powdr_amd import prover

    words = MALFORMED[what]
    (bc, spans), it = _planted(kind, words)
    pf, pf_logup, pf_segment, pf_segment_plain, flat = _well_formed_proofs()
    # column W itself is a next-row operand of the row layout public_programs_check speaks (constraints only): the other hooks refuse it
    if not (what == "column_W" and kind == "constraint"):
        assert prover.public_programs_check(MW, bc, spans, 0, it) is None
    else:
        assert prover.public_programs_check(MW, bc, spans, 0, it)["row_flags"] == 1
    for which in (0, 1):
        assert prover.jit_generated_sources(MW, bc, spans, it, which) == ([], 0)
    assert prover.verify_logup(pf_logup, MW, 2, bc, spans, it, num_queries=NQ, pow_bits=PB)[0] == 10
    assert sm.verify_logup(pf_logup, MW, 2, bc, spans, *it, num_queries=NQ, pow_bits=PB) == 10
    with pytest.raises(ValueError):
        sm.prove_logup(flat, MW, 2, bc, spans, *it, num_queries=NQ, pow_bits=PB)
    if kind == "constraint":
        assert prover.jit_generated_sources(MW, bc, spans, None, 0) == ([], 0)
        assert prover.verify(pf, MW, 2, bc, spans, num_queries=NQ, pow_bits=PB) == 10
        assert sm.verify(pf, MW, 2, bc, spans, num_queries=NQ, pow_bits=PB) == 10
        with pytest.raises(ValueError):
            sm.prove(flat, MW, 2, bc, spans, num_queries=NQ, pow_bits=PB)
    # the second AIR of a segment
    (gbc, gspans), git = _planted("constraint", [PA, 3])
    descs = [(MW, 2, gbc, gspans, git), (MW, 2, bc, spans, it)]
    airs = [(flat, MW, 2, gbc, gspans, git), (flat, MW, 2, bc, spans, it)]
    assert prover.verify_segment(descs, pf_segment, NQ, PB, True)[0] == 15
    assert sm.verify_segment(pf_segment, airs, num_queries=NQ, pow_bits=PB, logup=True)[0] == 15
    with pytest.raises(ValueError):
        sm.prove_segment(airs, num_queries=NQ, pow_bits=PB, logup=True)
    if kind == "constraint":  # (without LogUp a segment's interaction tables do not count, for either verifier)
        assert prover.verify_segment(descs, pf_segment_plain, NQ, PB, False)[0] == 15
        assert sm.verify_segment(pf_segment_plain, airs, num_queries=NQ, pow_bits=PB, logup=False)[0] == 15
        with pytest.raises(ValueError):
            sm.prove_segment(airs, num_queries=NQ, pow_bits=PB, logup=False)


def test_interaction_tables_outside_their_span_list_are_refused():
    """an interaction whose {multiplicity, arguments} run leaves the span list, and a span that leaves its bytecode"""
    from powdr_amd import prover

    (bc, spans), (inter, ispans, ibc) = _planted("constraint", [PA, 3])
    pf, pf_logup, _, _, flat = _well_formed_proofs()
    past_list = inter.copy()
    past_list[2, 1] = 3  # one argument more than the list holds
    past_bc = ispans.copy()
    past_bc[-1, 1] += 1
    cons_past_bc = spans.copy()
    cons_past_bc[-1, 1] += 1
    for it, sp in (((past_list, ispans, ibc), spans), ((inter, past_bc, ibc), spans), ((inter, ispans, ibc), cons_past_bc)):
        assert prover.public_programs_check(MW, bc, sp, 0, it) is None
        assert prover.verify_logup(pf_logup, MW, 2, bc, sp, it, num_queries=NQ, pow_bits=PB)[0] == 10
        assert sm.verify_logup(pf_logup, MW, 2, bc, sp, *it, num_queries=NQ, pow_bits=PB) == 10
        with pytest.raises(ValueError):
            sm.prove_logup(flat, MW, 2, bc, sp, *it, num_queries=NQ, pow_bits=PB)
    with pytest.raises(ValueError):
        sm.group_starts(past_list, ispans, ibc)
    with pytest.raises(ValueError):
        prover.logup_group_starts((past_list, ispans, ibc))


@pytest.mark.parametrize("kind", SPAN_KINDS)
def test_depth_16_is_accepted_by_the_product_and_by_the_oracle(kind):
    """one slot below the refusals above: a right-leaning sum of 16 columns fills the evaluation stack exactly. Both sides accept it,
    the trace satisfies it (column 0 = minus the other fifteen), and both verifiers accept the oracle's proofs."""
    from powdr_amd import prover

    words = _chain_words(16)
    assert ra.STACK_CAPACITY == 16
    (bc, spans), it = _planted(kind, words)
    chk = prover.public_programs_check(MW, bc, spans, 0, it)
    assert chk is not None and chk["max_degree"] == 2
    for which in (0, 1):
        assert len(prover.jit_generated_sources(MW, bc, spans, it, which)[0]) >= 1
    T = np.random.default_rng(16).integers(0, P, (MW, 8)).astype(np.int64)
    T[4] = 0                                   # the sibling constraints: col_0 col_1 - col_2, col_3^2, col_4
    if kind == "constraint":
        T[1], T[2] = 0, 0
        T[0] = -T[1:16].sum(axis=0) % P        # the planted sum of columns 0 .. 15
    else:
        T[3], T[2] = 0, T[0] * T[1] % P
    flat = T.astype(np.uint32).reshape(-1)
    pf = sm.prove(flat, MW, 3, bc, spans, num_queries=NQ, pow_bits=PB)
    assert prover.verify(pf, MW, 3, bc, spans, num_queries=NQ, pow_bits=PB) == sm.verify(pf, MW, 3, bc, spans, num_queries=NQ, pow_bits=PB) == 0
    pf = sm.prove_logup(flat, MW, 3, bc, spans, *it, num_queries=NQ, pow_bits=PB)
    assert prover.verify_logup(pf, MW, 3, bc, spans, it, num_queries=NQ, pow_bits=PB)[0] == 0
    assert sm.verify_logup(pf, MW, 3, bc, spans, *it, num_queries=NQ, pow_bits=PB) == 0
    airs = [(flat, MW, 3, bc, spans, it)]
    pf = sm.prove_segment(airs, num_queries=NQ, pow_bits=PB, logup=True)
    assert prover.verify_segment([(MW, 3, bc, spans, it)], pf, NQ, PB, True)[0] == sm.verify_segment(pf, airs, num_queries=NQ, pow_bits=PB, logup=True)[0] == 0
