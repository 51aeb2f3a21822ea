"""Random AIRs for the proof tests (numpy only; importable without a GPU): one seeded generator shared by test_random_airs_cpu.py and
test_random_airs_gpu.py.

random_air(seed) -> (W, (bc, spans), (inter, ispans, ibc), meta), deterministic in the seed, every seed a case: expression trees are
built top-down under a degree budget (a MUL splits what is left between its children), so nothing is generated and thrown away.
Constraints and multiplicities have degree <= 3, arguments degree <= 2: the bounds logup_group_starts packs under. Shapes the
plan-time compilers and the kernels treat specially are planted on purpose (PLANTS); `meta` says what a case contains.

derived_air(seed, ...) builds AIRs that are SATISFIED by construction (free columns, every further column defined by an expression of
earlier ones, the constraint col_j - E_j, a bus that balances), optionally over the row layout of logup_groups.hpp `postfix_row_flags`
(next-row reads, row selectors, preprocessed columns, public values).

Every expected value in here (cells, violations, bus tuples) is this file's own evaluation of its own trees with Python / uint64
modular arithmetic: no product code, no oracle."""
import numpy as np

from oracle import apc_model as om
from tests import _edge_values as ev
from tests._edge_values import _programs

P = om.P
PA, PC, ADD, SUB, MUL, NEG = om.OP_PUSH_APC, om.OP_PUSH_CONST, om.OP_ADD, om.OP_SUB, om.OP_MUL, om.OP_NEG
STACK_CAPACITY = 16  # POWDR_EXPR_STACK_CAPACITY: the deepest program a prover accepts

_EDGE_BASE = [0, 1, 2, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2]
EDGE_CONSTANTS = _EDGE_BASE + [ev.word(v) for v in _EDGE_BASE]

# ---------------------------------------------------------------------------------------------------------------- trees
# ("col", c) | ("const", v) | ("neg", a) | ("add" | "sub" | "mul", a, b)
_BIN = {"add": ADD, "sub": SUB, "mul": MUL}


def col(c):
    return ("col", int(c))


def const(v):
    return ("const", int(v) % P)


def emit(t):
    """post-fix words of a tree"""
    if t[0] == "col":
        return [PA, t[1]]
    if t[0] == "const":
        return [PC, t[1]]
    if t[0] == "neg":
        return emit(t[1]) + [NEG]
    return emit(t[1]) + emit(t[2]) + [_BIN[t[0]]]


def degree(t):
    """syntactic degree in the columns (what postfix_degree computes: x * 0 has degree 1); operands from `t`'s own W on are not known
    here: derived_air computes its degrees itself"""
    if t[0] in ("col", "const"):
        return 1 if t[0] == "col" else 0
    if t[0] == "neg":
        return degree(t[1])
    a, b = degree(t[1]), degree(t[2])
    return a + b if t[0] == "mul" else max(a, b)


def stack_depth(t):
    """values on the evaluation stack at the deepest point of the post-fix program"""
    if t[0] in ("col", "const"):
        return 1
    if t[0] == "neg":
        return stack_depth(t[1])
    return max(stack_depth(t[1]), 1 + stack_depth(t[2]))


def evaluate(t, T):
    """the tree on every row at once: T is (operands x rows) canonical; uint64 holds a product of two words"""
    p = np.uint64(P)
    if t[0] == "col":
        return np.asarray(T[t[1]], dtype=np.uint64)
    if t[0] == "const":
        return np.full(np.asarray(T).shape[1], t[1], np.uint64)
    if t[0] == "neg":
        return (p - evaluate(t[1], T)) % p
    a, b = evaluate(t[1], T), evaluate(t[2], T)
    return (a + b) % p if t[0] == "add" else (a + p - b) % p if t[0] == "sub" else a * b % p


def _leaf(rng, W, deg):
    r = rng.random()
    if deg >= 1 and r < 0.6:
        return col(rng.integers(0, W))
    if r < 0.8:
        return const(rng.integers(0, P))
    return const(EDGE_CONSTANTS[rng.integers(0, len(EDGE_CONSTANTS))])


def random_tree(rng, W, deg, leaves):
    """a tree of degree <= deg with at most `leaves` leaves (so its stack depth is at most `leaves`)"""
    if leaves <= 1 or rng.random() < 0.12:
        return _leaf(rng, W, deg)
    op = ["add", "sub", "mul", "neg"][rng.choice(4, p=[0.3, 0.25, 0.33, 0.12])]
    if op == "neg":
        return ("neg", random_tree(rng, W, deg, leaves))
    left = int(rng.integers(1, leaves))
    if op == "mul":
        da = int(rng.integers(0, deg + 1))  # the MUL splits the remaining degree between its children
        return ("mul", random_tree(rng, W, da, left), random_tree(rng, W, deg - da, leaves - left))
    return (op, random_tree(rng, W, deg, left), random_tree(rng, W, deg, leaves - left))


def chain(rng, W, depth, columns_only=False):
    """right-leaning x0 +- (x1 +- (x2 ...)) of `depth` leaves: every leaf is pushed before the first operator runs: stack depth `depth`"""
    leaf = (lambda: col(rng.integers(0, W))) if columns_only else (lambda: _leaf(rng, W, 1))
    t = leaf()
    for _ in range(depth - 1):
        t = ("add" if rng.random() < 0.5 else "sub", leaf(), t)
    assert stack_depth(t) == depth
    return t


# ---------------------------------------------------------------------------------------------------------------- random AIRs
PLANTS = ["chain15_constraint", "chain16_constraint", "chain15_multiplicity", "chain16_multiplicity", "chain15_argument", "chain16_argument",
          "neg_neg", "mul_zero", "mul_one", "zero_minus", "const_fold", "constant_only_arguments", "identical_arguments",
          "constant_multiplicity_p_minus_1", "no_constraints", "no_interactions"]
_BUSES = [1, 2, 7, 0x7fff]


def random_air(seed: int):
    """(W, (bc, spans), (inter, ispans, ibc), meta); meta = dict(seed, W, plants: set of PLANTS, constraint_degrees, max_degree,
    multiplicity_degrees, argument_degrees (per interaction: the highest), n_args, max_stack_depth, constraints / interactions: the trees,
    homogeneous: every constraint vanishes on an all-zero row - half of the AIRs, so that a trace with zero rows has clean rows)"""
    rng = np.random.default_rng([0x52414952, seed])
    # W from 1 to 70: seeds 0..3 pin the four residues mod 4 around the 64-column openings tile and the smallest width
    W = [1, 66, 67, 64][seed] if seed < 4 else [65, 70][seed - 4] if seed < 6 else int(rng.integers(1, 71))
    plants = {p for p in PLANTS if rng.random() < 0.3}
    if "no_constraints" in plants and "no_interactions" in plants:  # an AIR proves something
        plants.discard("no_interactions")
    x = lambda: col(rng.integers(0, W))
    homogeneous = bool(rng.random() < 0.5)
    constraints, interactions = [], []
    if "no_constraints" not in plants:
        for _ in range(int(rng.integers(1, 9))):
            deg, leaves = int(rng.integers(1, 4)), int(rng.integers(1, 13))
            constraints.append(("mul", x(), random_tree(rng, W, deg - 1, leaves)) if homogeneous else random_tree(rng, W, deg, leaves))
        if "chain15_constraint" in plants:
            constraints.append(chain(rng, W, 15, homogeneous))
        if "chain16_constraint" in plants:
            constraints.insert(0, chain(rng, W, 16, homogeneous))
        if "neg_neg" in plants:
            constraints.append(("neg", ("neg", ("mul", x(), x()))))
        if "mul_zero" in plants:
            constraints.append(("add", ("mul", x(), const(0)), x()))
        if "mul_one" in plants:
            constraints.append(("sub", ("mul", x(), const(1)), ("mul", const(1), x())))
        if "zero_minus" in plants:
            constraints.append(("sub", const(0), ("mul", x(), x())))
        if "const_fold" in plants:  # c1 * c2 - c3: what xbc folds into one constant
            constraints.append(("mul" if homogeneous else "add", x(), ("sub", ("mul", const(rng.integers(0, P)), const(P - 2)), const(ev.word(P - 1)))))
    plants -= {p for p in plants if "no_constraints" in plants and p in ("chain15_constraint", "chain16_constraint", "neg_neg", "mul_zero", "mul_one",
                                                                         "zero_minus", "const_fold")}
    if "no_interactions" not in plants:
        def multiplicity():
            r = rng.random()
            if r < 0.45:
                return x()
            if r < 0.55:  # (degree 3: such an interaction packs alone)
                return ("mul", x(), ("sub", ("mul", x(), x()), _leaf(rng, W, 1)))
            return random_tree(rng, W, 3, int(rng.integers(1, 7))) if r < 0.9 else const(rng.integers(0, P))
        for _ in range(int(rng.integers(1, 9))):
            n_args = int(rng.integers(0, 8))  # 0..7 arguments
            interactions.append((_BUSES[rng.integers(0, len(_BUSES))], multiplicity(),
                                 [x() if rng.random() < 0.6 else random_tree(rng, W, 2, int(rng.integers(1, 6))) for _ in range(n_args)]))
        for d in (15, 16):
            if f"chain{d}_multiplicity" in plants:
                interactions.append((3, chain(rng, W, d), [x()]))
            if f"chain{d}_argument" in plants:
                interactions.append((3, x(), [x(), chain(rng, W, d)]))
        if "constant_only_arguments" in plants:  # degree-0 denominators: any number of them shares a group (here: at least three)
            for _ in range(int(rng.integers(3, 6))):
                interactions.append((5, x(), [const(EDGE_CONSTANTS[rng.integers(0, len(EDGE_CONSTANTS))]) for _ in range(int(rng.integers(1, 4)))]))
        if "identical_arguments" in plants:
            same = [x(), x()]
            interactions += [(6, x(), same), (6, x(), same)]
        if "constant_multiplicity_p_minus_1" in plants:
            interactions.append((6, const(P - 1), [x()]))
    else:
        plants -= {p for p in plants if p.endswith(("_multiplicity", "_argument", "_arguments", "_p_minus_1"))}
    cons, it = _programs([emit(c) for c in constraints], [(bus, emit(m), [emit(a) for a in args]) for bus, m, args in interactions])
    trees = constraints + [m for _, m, _ in interactions] + [a for _, _, args in interactions for a in args]
    meta = dict(seed=seed, W=W, plants=plants, homogeneous=homogeneous, constraints=constraints, interactions=interactions,
                constraint_degrees=[degree(c) for c in constraints], max_degree=max([degree(c) for c in constraints], default=0),
                multiplicity_degrees=[degree(m) for _, m, _ in interactions],
                argument_degrees=[max([degree(a) for a in args], default=0) for _, _, args in interactions],
                n_args=[len(args) for _, _, args in interactions], max_stack_depth=max(stack_depth(t) for t in trees))
    assert all(d <= 3 for d in meta["constraint_degrees"] + meta["multiplicity_degrees"]) and all(d <= 2 for d in meta["argument_degrees"])
    assert meta["max_stack_depth"] <= STACK_CAPACITY
    return W, cons, it, meta


def group_sizes(starts):
    return np.diff(np.asarray(starts, dtype=np.int64)).tolist()


def multiplicity_columns(meta):
    """the columns the multiplicity trees read"""
    out = set()

    def walk(t):
        if t[0] == "col":
            out.add(t[1])
        elif t[0] != "const":
            for s in t[1:]:
                walk(s)
    for _, m, _ in meta["interactions"]:
        walk(m)
    return sorted(out)


# ---------------------------------------------------------------------------------------------------------------- traces
TRACE_KINDS = ["uniform", "edge_columns", "zero_multiplicity_block", "zero_rows"]


def trace_matrix(meta, log_h: int, kind: str, n_rows: int = None) -> np.ndarray:
    """W x H canonical (n_rows: a height that is no power of two, for the generated code on the host).
    uniform; edge_columns: one all-zero and one all-(p-1) column (W >= 2); zero_multiplicity_block: rows H/4 .. H/2 (at least one) with
    every column a multiplicity reads at zero; zero_rows: the last third of the rows (at least one) all zero."""
    W, H = meta["W"], n_rows if n_rows is not None else 1 << log_h
    rng = np.random.default_rng([0x54524143, meta["seed"], H, TRACE_KINDS.index(kind)])
    t = rng.integers(0, P, (W, H)).astype(np.uint32)
    if kind == "edge_columns" and W >= 2:
        a, b = rng.choice(W, 2, replace=False)
        t[a], t[b] = 0, P - 1
    elif kind == "zero_multiplicity_block":
        t[multiplicity_columns(meta), H // 4:max(H // 2, H // 4 + 1)] = 0
    elif kind == "zero_rows":
        t[:, H - max(H // 3, 1):] = 0
    return np.ascontiguousarray(t)


def trace(meta, log_h: int, kind: str) -> np.ndarray:
    """flat column-major canonical uint32"""
    return trace_matrix(meta, log_h, kind).reshape(-1)


def violations(constraints, T):
    """(number of violated (row, constraint) pairs, number of violating rows, (row, constraint) of the first in row-major order or None)"""
    if not constraints:
        return 0, 0, None
    bad = np.stack([evaluate(c, T) for c in constraints]) != 0  # constraints x rows
    rows = np.flatnonzero(bad.any(axis=0))
    first = None if not len(rows) else (int(rows[0]), int(np.argmax(bad[:, rows[0]])))
    return int(bad.sum()), len(rows), first


def vanishing_multiplicity_rows(meta, T):
    """the rows on which every multiplicity is zero"""
    if not meta["interactions"]:
        return np.zeros(0, np.int64)
    return np.flatnonzero(np.all(np.stack([evaluate(m, T) for _, m, _ in meta["interactions"]]) == 0, axis=0))


def bus_tally(interactions, T):
    """{(bus, args): net multiplicity mod p} without the tuples whose multiplicities cancel: what a balanced bus leaves empty"""
    tally = {}
    for bus, m, args in interactions:
        ms = evaluate(m, T).tolist()
        cols = [evaluate(a, T).tolist() for a in args]
        for r, mu in enumerate(ms):
            if mu:
                key = (bus, tuple(c[r] for c in cols))
                tally[key] = (tally.get(key, 0) + mu) % P
    return {k: v for k, v in tally.items() if v}


# ---------------------------------------------------------------------------------------------------------------- derived AIRs
DERIVED_BUS = 11


def derived_air(seed: int, log_h: int, row_aware: bool = False):
    """An AIR its trace satisfies by construction. k free uniform columns; every further column j = E_j(earlier columns), degree <= 2;
    constraint j: col_j - E_j. One bus that balances: every send (multiplicity 1, the tuple of some columns at row r) is paired with a
    receive (multiplicity p - 1) of the same tuple from columns that hold the send's columns on the permuted row.

    row_aware: operands over the row layout of W1 = W + pre_width columns (c < W1: this row; W1 + c: the next row; 2 W1, 2 W1 + 1,
    2 W1 + 2: is_first_row, is_last_row, is_transition; 2 W1 + 3 + k: public value k). E_j may then be
      * an expression of EARLIER columns on the next row: the constraint is is_transition * (col_j - E_j), the last row's cell is free;
      * an expression of preprocessed columns and public values;
    and two boundary constraints tie public values to cells: is_first_row * (col_0 - pub_0), is_last_row * (col_1 - pub_1).

    -> dict(W, cons=(bc, spans), it, T: W x H canonical, pre: pre_width x H or None, pre_width, public: values or None, transition,
            constraints: [(kind, column)], interactions: trees over main columns, check(T, pre, public) -> violations() of the whole
            system under this file's evaluation)"""
    rng = np.random.default_rng([0x44455249, seed, int(row_aware)])
    H = 1 << log_h
    k = int(rng.integers(2, 5))
    n_derived = int(rng.integers(2, 7))
    pre_width = int(rng.integers(1, 4)) if row_aware else 0
    n_public = 3 if row_aware else 0
    # layout of the main columns: free | derived | bus copies (filled below)
    n_bus = int(rng.integers(1, 4))                     # send/receive pairs
    arity = [int(rng.integers(1, 4)) for _ in range(n_bus)]
    W = k + n_derived + sum(arity)
    W1 = W + pre_width
    F, L, TR, PUB = 2 * W1, 2 * W1 + 1, 2 * W1 + 2, 2 * W1 + 3
    pre = rng.integers(0, P, (pre_width, H)).astype(np.uint64) if pre_width else None
    public = rng.integers(0, P, n_public).astype(np.uint64) if n_public else None
    T = np.zeros((W, H), np.uint64)
    T[:k] = rng.integers(0, P, (k, H))

    def operands(T_):
        """the operand matrix the constraint trees are evaluated over: this row | next row | selectors | public values"""
        if not row_aware:
            return T_
        cur = np.concatenate([T_, pre]) if pre_width else T_
        sel = np.zeros((3, H), np.uint64)
        sel[0, 0], sel[1, H - 1], sel[2, :H - 1] = 1, 1, 1  # (is_transition: any non-zero value off the last row; 1 in this evaluation)
        return np.concatenate([cur, np.roll(cur, -1, axis=1), sel, np.repeat(public[:, None], H, axis=1)])

    constraints, kinds = [], []
    for j in range(k, k + n_derived):
        mode = str(rng.choice(["row", "next", "fixed"])) if row_aware else "row"
        if mode == "row":
            E = random_tree(rng, j, 2, int(rng.integers(1, 6)))
            T[j] = evaluate(E, T)
            c = ("sub", col(j), E)
        elif mode == "next":  # earlier columns on the next row
            E = _shift(random_tree(rng, j, 2, int(rng.integers(1, 5))), W1)
            T[j] = evaluate(E, operands(T))
            T[j, H - 1] = rng.integers(0, P)  # (free: the constraint does not hold the last row)
            c = ("mul", col(TR), ("sub", col(j), E))
        else:                 # preprocessed columns and public values
            E = ("add", ("mul", col(W + int(rng.integers(0, pre_width))), col(PUB + 2)), random_tree(rng, j, 1, 2))
            T[j] = evaluate(E, operands(T))
            c = ("sub", col(j), E)
        constraints.append(c)
        kinds.append((mode, j))
    interactions, base = [], k + n_derived
    perm = rng.permutation(H)
    for a in arity:
        src = [int(rng.integers(0, k + n_derived)) for _ in range(a)]
        dst = list(range(base, base + a))
        base += a
        for s, d in zip(src, dst):
            T[d, perm] = T[s]  # the receive on row perm[r] carries the send of row r
        interactions += [(DERIVED_BUS, const(1), [col(s) for s in src]), (DERIVED_BUS, const(P - 1), [col(d) for d in dst])]
    if row_aware:
        public[0], public[1] = T[0, 0], T[1, H - 1]
        constraints += [("mul", col(F), ("sub", col(0), col(PUB))), ("mul", col(L), ("sub", col(1), col(PUB + 1)))]
        kinds += [("first", 0), ("last", 1)]
    cons, it = _programs([emit(c) for c in constraints], [(bus, emit(m), [emit(x) for x in args]) for bus, m, args in interactions])

    def check(T_, public_=None):
        ops = operands(np.asarray(T_, dtype=np.uint64)) if public_ is None else _with_public(operands, T_, public, public_)
        return violations(constraints, ops)

    return dict(W=W, cons=cons, it=it, T=T.astype(np.uint32), pre=None if pre is None else pre.astype(np.uint32), pre_width=pre_width,
                public=None if public is None else public.astype(np.uint32), transition=row_aware, constraints=constraints, kinds=kinds,
                interactions=interactions, check=check, log_h=log_h)


def _with_public(operands, T_, public, values):
    keep = public.copy()
    public[:] = np.asarray(values, dtype=np.uint64)
    try:
        return operands(np.asarray(T_, dtype=np.uint64))
    finally:
        public[:] = keep


def _shift(t, by):
    """every column operand of a tree moved by `by` (this row -> the next row)"""
    if t[0] == "col":
        return col(t[1] + by)
    if t[0] == "const":
        return t
    return (t[0],) + tuple(_shift(s, by) for s in t[1:])
