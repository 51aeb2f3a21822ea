"""Edge-valued traces for the proof tests (numpy only; importable without a GPU).

The expression and opening kernels centre and multiply the MONTGOMERY word of a cell, the protocol speaks of its canonical value:
both views get their extremes. word(w) is the canonical value whose device word is w. The table CASES x kinds(air) is what
test_edge_values_cpu.py validates on the CPU and what a GPU proof test of these traces iterates; expected_code() holds the verifiers'
answer for each entry, computed here from the constraint programs with plain integer arithmetic (no oracle, no product code)."""
import zlib

import numpy as np

from oracle import apc_model as om
from tests._jit_host import eval_postfix  # noqa: F401  (a post-fix program on one row, plain Python integers: the tests use it from here)

P = om.P
PA, PC, ADD, SUB, MUL, NEG = om.OP_PUSH_APC, om.OP_PUSH_CONST, om.OP_ADD, om.OP_SUB, om.OP_MUL, om.OP_NEG
_R_INV = pow((1 << 32) % P, -1, P)


def word(w: int) -> int:
    """the canonical value whose Montgomery (device) word is w: w * R^-1 mod p, R = 2^32"""
    return (w * _R_INV) % P


EDGE_NAMES = ["0", "1", "p-1", "(p-1)/2", "(p+1)/2", "word(1)", "word(p-1)", "word((p-1)/2)", "word((p+1)/2)"]
EDGE = np.array([0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, word(1), word(P - 1), word((P - 1) // 2), word((P + 1) // 2)], np.uint32)
CHALLENGE_WORDS = [(P - 1) // 2, (P + 1) // 2, P - 1, 1]  # device words of the extreme challenges (test 2b)


# ---------------------------------------------------------------------------------------------------------------- AIRs
def _programs(constraints, interactions):
    """[post-fix program], [(bus, multiplicity program, [argument programs])] -> ((bc, spans), (inter, ispans, ibc))"""
    bc, spans, ibc, ispans, inter = [], [], [], [], []

    def span(words, sink, spans_):
        spans_.append((len(sink), len(words)))
        sink.extend(words)

    for c in constraints:
        span(c, bc, spans)
    for bus, mult, args in interactions:
        inter.append((bus, len(args), len(ispans)))
        span(mult, ibc, ispans)
        for a in args:
            span(a, ibc, ispans)
    return ((np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)),
            (np.array(inter, np.uint32).reshape(-1, 3), np.array(ispans, np.uint32).reshape(-1, 2), np.array(ibc, np.uint32)))


WIDE_W = 67  # one full 64-column tile of the openings kernel + 3; W % 4 == 3: the leftover columns of the DEEP kernels
WIDE_BUS = 9
WIDE_CANCEL = (16, 17)  # multiplicity columns of the two interactions with identical arguments (one LogUp group)


def wide_air():
    """W = 67. Five degree-2 constraints, one linear constraint over all 67 columns (Horner in word(p-1): stack depth 2), interactions
    with 0 .. 5 arguments on one bus (every parity of the denominators' two-product reduction cadence), two interactions with the same
    arguments that share a group (`cancel`), one with the constant multiplicity p - 1."""
    col = lambda c: [PA, c]
    k = word(P - 1)
    horner = col(0)
    for c in range(1, WIDE_W):
        horner += [PC, k, MUL] + col(c) + [ADD]
    constraints = [
        col(0) + col(1) + [MUL] + col(2) + [SUB],                                     # a*b - c
        col(3) + col(3) + [PC, 1, SUB, MUL],                                          # d*(d-1)
        col(0) + col(1) + [ADD] + col(2) + col(3) + [ADD, MUL] + col(4) + [NEG, ADD],  # (a+b)*(c+d) - e
        col(64) + col(65) + [MUL] + col(66) + [SUB],                                  # the last three columns
        col(5) + col(6) + [MUL] + col(7) + col(8) + [MUL, ADD],                       # two products
        horner,
    ]
    same = [col(30), col(31)]
    interactions = [
        (WIDE_BUS, col(WIDE_CANCEL[0]), same),                    # these two and the argument-less one: a group of three
        (WIDE_BUS, col(WIDE_CANCEL[1]), same),
        (WIDE_BUS, col(10), []),
        (WIDE_BUS, col(11), [col(20)]),
        (WIDE_BUS, col(12), [col(21), col(22)]),
        (WIDE_BUS, col(13), [col(23), col(24), col(66)]),
        (WIDE_BUS, col(14), [col(25), col(26), col(27), col(28)]),
        (WIDE_BUS, col(15), [col(32), col(33), col(34), col(35), col(36)]),
        (WIDE_BUS, [PC, P - 1], [col(40)]),
    ]
    cons, it = _programs(constraints, interactions)
    return WIDE_W, cons, it


def one_air():
    """W = 1, no constraints, one interaction (bus, [PA 0], [[PA 0]])"""
    cons, it = _programs([], [(2, [PA, 0], [[PA, 0]])])
    return 1, cons, it


def air_tables(air: str):
    """(W, (bc, spans), (inter, ispans, ibc))"""
    if air == "hand":
        from tests.test_jit import hand_made_air

        return hand_made_air()
    return {"wide": wide_air, "one": one_air}[air]()


AIRS = ["hand", "wide", "one"]
HEIGHTS = [1, 2, 8, 12, 13]  # one lane pair, ..., one 256-lane block, one and two chunks of the LogUp prefix scan
DEEP_COMBO_LOG_HEIGHT = 16   # from here on the DEEP numerator is combined on the un-extended matrices (`hand` only)
CASES = [(air, log_h) for air in AIRS for log_h in HEIGHTS]
NUM_QUERIES, POW_BITS = 4, 0


def multiplicity_columns(air: str):
    """the columns the multiplicity programs read"""
    _, _, (inter, ispans, ibc) = air_tables(air)
    cols = set()
    for _, _, s0 in inter.tolist():
        off, ln = ispans[s0].tolist()
        code = ibc[off:off + ln].tolist()
        i = 0
        while i < len(code):
            if code[i] in (PA, PC):
                if code[i] == PA:
                    cols.add(code[i + 1])
                i += 2
            else:
                i += 1
    return sorted(cols)


# ---------------------------------------------------------------------------------------------------------------- trace kinds
SATISFYING_KINDS = ("const[0]", "satisfied")  # the kinds on which every constraint of their AIR holds on every row


def kinds(air: str):
    ks = [f"const[{n}]" for n in EDGE_NAMES] + ["const_by_column", "cells", "runs4", "runs16", "spike_first", "spike_last", "all_padding"]
    if air == "wide":
        ks.append("cancel")     # needs two interactions with identical arguments in one group: only `wide` has them
    if air == "hand":
        ks.append("satisfied")
    return ks


def _cells(rng, W, H):
    return EDGE[rng.integers(0, len(EDGE), (W, H))]


def matrix(kind: str, W: int, H: int, seed: int, air: str = None) -> np.ndarray:
    """W x H canonical words of one trace kind (H need not be a power of two: test 2b uses 24 rows); the kinds that speak of an
    AIR's columns (`all_padding`, `cancel`, `satisfied`) need `air`."""
    rng = np.random.default_rng(seed)
    t = np.zeros((W, H), np.uint32)
    if kind.startswith("const["):
        t[:] = EDGE[EDGE_NAMES.index(kind[6:-1])]
    elif kind == "const_by_column":
        t[:] = EDGE[np.arange(W) % 9][:, None]
    elif kind == "cells":
        t = _cells(rng, W, H)
    elif kind in ("runs4", "runs16"):
        run = int(kind[4:])
        t[:] = np.where((np.arange(H) // run) % 2 == 0, word((P - 1) // 2), word((P + 1) // 2)).astype(np.uint32)[None, :]
    elif kind in ("spike_first", "spike_last"):
        t[:, 0 if kind == "spike_first" else H - 1] = EDGE[rng.integers(0, len(EDGE), W)]
    elif kind == "all_padding":
        t = _cells(rng, W, H)
        t[multiplicity_columns(air)] = 0
    elif kind == "cancel":
        assert air == "wide"
        t = _cells(rng, W, H)
        t[WIDE_CANCEL[0]], t[WIDE_CANCEL[1]] = 1, P - 1
    elif kind == "satisfied":
        assert air == "hand"
        t = _cells(rng, W, H)
        t[0], t[1], t[2] = P - 1, P - 1, 1
        t[3] = rng.integers(0, 2, H)
        t[4] = ((t[0].astype(np.uint64) + t[1]) * (t[2].astype(np.uint64) + t[3]) % P).astype(np.uint32)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(t, dtype=np.uint32)


def _seed(air, kind, log_h):
    return zlib.crc32(f"{air}/{kind}/{log_h}".encode())


def trace(air: str, kind: str, log_h: int) -> np.ndarray:
    """flat column-major canonical uint32"""
    W = air_tables(air)[0]
    return matrix(kind, W, 1 << log_h, _seed(air, kind, log_h), air).reshape(-1)


TRACE_KINDS = {k: (lambda W, log_h, seed, _k=k: matrix(_k, W, 1 << log_h, seed).reshape(-1))
               for k in [f"const[{n}]" for n in EDGE_NAMES] + ["const_by_column", "cells", "runs4", "runs16", "spike_first", "spike_last"]}


# ---------------------------------------------------------------------------------------------------------------- expected codes
def eval_postfix_columns(code, T):
    """the same on every row at once: T is W x H canonical; uint64 holds a product of two words"""
    T = np.asarray(T, dtype=np.uint64)
    p = np.uint64(P)
    st, i = [], 0
    while i < len(code):
        op = int(code[i])
        if op in (PA, PC):
            st.append(T[int(code[i + 1])] if op == PA else np.full(T.shape[1], int(code[i + 1]) % P, np.uint64))
            i += 2
        elif op == NEG:
            st.append((p - st.pop()) % p)
            i += 1
        else:
            y, x = st.pop(), st.pop()
            st.append((x + y) % p if op == ADD else (x + p - y) % p if op == SUB else x * y % p)
            i += 1
    assert len(st) == 1
    return st[0]


def first_violation(air: str, flat):
    """(row, constraint) of the first violated constraint in row-major order, or None"""
    W, (bc, spans), _ = air_tables(air)
    T = np.asarray(flat).reshape(W, -1)
    vals = [eval_postfix_columns(bc[off:off + ln].tolist(), T) for off, ln in spans.tolist()]
    if not vals:
        return None
    bad = np.stack(vals) != 0  # constraints x rows
    rows = np.flatnonzero(bad.any(axis=0))
    if not len(rows):
        return None
    return int(rows[0]), int(np.argmax(bad[:, rows[0]]))


_CODES = {}


def expected_code(air: str, kind: str, log_h: int) -> int:
    """what verify / verify_logup answer for a proof of this trace: 0 where every constraint holds on every row, else 2 (the constraint
    identity at the out-of-domain point; a bus sum that does not vanish is no error of a single AIR). Computed from the constraint
    programs, not from the kind's name: test_edge_values_cpu.py holds it against SATISFYING_KINDS. `all_padding` is NOT a zero trace:
    only its multiplicity columns are zero (no row of the LogUp phase inverts anything), the other cells are the `cells` draw, so it
    violates the constraints of `hand` and `wide` like `cells` does (2); the all-zero trace is const[0] (0)."""
    key = (air, kind, log_h)
    if key not in _CODES:
        _CODES[key] = 0 if first_violation(air, trace(air, kind, log_h)) is None else 2
    return _CODES[key]
