"""The memory Merkle AIR without a GPU (powdr_amd/memory_tree.py merkle_air, system_airs.boundary_air(leaf_bus=)): its
shape, the defaults it must not move, and — on the numpy reference trace of tests/_memory_merkle_ref.py, with a numpy stand-in for the
boundary AIR's leaf sends and tests/_poseidon2_air_ref rows as the chip — that the honest trace of every leaf set at height 3 satisfies
every constraint and closes buses 5, 8 and 9, and that each tampering of the soundness argument's list is caught by the constraint or
bus the argument names."""
import itertools

import numpy as np
import pytest

from tests import _memory_merkle_ref as mref
from tests import _memory_tree_ref as tref

P = mref.P
EDGE_KEYS_30 = [0, 1, 1 << 29, (1 << 30) - 1]


@pytest.fixture(scope="module")
def mt():
    from powdr_amd import memory_tree

    return memory_tree


@pytest.fixture(scope="module")
def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


def leaf_words(rng, n):
    """n payloads as the boundary AIR has them: four words, then four zeros"""
    w = np.zeros((n, 8), np.uint32)
    w[:, :4] = rng.integers(0, 256, (n, 4))
    return w


class Case:
    """one update of a tree of height `height` that holds `stored` leaves: the reference trace, its public values and the AIRs around it"""

    def __init__(self, mt, constants, height, stored, keys, seed, log_height=None):
        rng = np.random.default_rng(seed)
        self.constants, self.height, self.stored, self.seed = constants, height, list(stored), seed
        tree = tref.SparseTree(height, constants)
        tree.write(stored, leaf_words(rng, len(stored)))
        self.keys = sorted(keys)
        self.init = np.array([tree.payload.get(k, np.zeros(8, np.uint32)) for k in self.keys], np.uint32)
        self.fin = leaf_words(rng, len(self.keys))
        self.root_before = tree.root().copy()
        records, ids, _, n_rows = tree.update(self.keys, self.init, self.fin)
        self.root_after = tree.root().copy()
        self.cols, self.where = mref.trace(records, ids, n_rows, height, log_height)
        self.public = mref.public_of(self.cols)
        self.air = mt.merkle_air(height)
        self.names = [n for n, _ in mt.merkle_constraints(height)]
        self.leaves = mref.leaf_sender(self.keys, self.init, self.fin)

    def violations(self, cols=None, public=None):
        return mref.violations(self.air, self.names, self.cols if cols is None else cols, self.public if public is None else public)

    def unbalanced(self, cols=None):
        return self.caught(self.cols if cols is None else cols)[1]

    def caught(self, cols, public=None):
        """(names of the violated constraints, unbalanced buses) with the chip remade for what the trace now asks"""
        cells, inter = mref.chip(cols, self.constants)
        return set(self.violations(cols, public)), mref.unbalanced([self.leaves, (list(cols), self.air.inter), (list(cells), inter)])


# ---- the AIR ------------------------------------------------------------------------------------------------------------------------------
def test_the_air_has_55_columns_16_public_values_and_degree_at_most_3(mt):
    from powdr_amd import prover

    air = mt.merkle_air()
    assert air.width == 55 == len(mt.MERKLE_COLUMNS) == mref.WIDTH and air.n_public == 16 == len(mt.MERKLE_PUBLIC) and air.transition
    assert mt.MERKLE_COLUMNS[:7] == ["valid", "is_root", "is_leaf", "left_touched", "right_touched", "level", "index"]
    assert [mt.MERKLE_COLUMNS.index(f"{n}_0") for n in ("left0", "right0", "out0", "left1", "right1", "out1")] == [mref.LEFT0, mref.RIGHT0, mref.OUT0, mref.LEFT1,
                                                                                                                 mref.RIGHT1, mref.OUT1]
    assert mt.MERKLE_PUBLIC == [f"root_before{j}" for j in range(8)] + [f"root_after{j}" for j in range(8)]
    got = prover.public_programs_check(air.width, air.cons[0], air.cons[1], air.n_public, air.inter)
    assert got is not None and got["max_degree"] <= 3
    assert got["row_flags"] & 1 and got["row_flags"] & 2  # a next row is read (is_root'), and a row selector
    assert len(air.cons[1]) == len(mt.merkle_constraints(30))
    inter = np.asarray(air.inter[0]).tolist()
    assert [(b, n) for b, n, _ in inter] == [(5, 24), (5, 24), (8, 18), (8, 18), (8, 18), (9, 9)]
    # public values are not allowed in interaction programs: every operand of theirs is a main column
    bc, i = np.asarray(air.inter[2]).tolist(), 0
    while i < len(bc):
        assert bc[i] != 0 or bc[i + 1] < air.width
        i += 2 if bc[i] in (0, 1) else 1
    # the buses are parameters
    other = mt.merkle_air(7, compress_bus=11, merkle_bus=12, leaf_bus=13)
    assert sorted(set(np.asarray(other.inter[0])[:, 0].tolist())) == [11, 12, 13]
    assert mt.memory_links(4) == [(4, 8 + j, 4, j) for j in range(8)]


def test_defaults_and_refusals(mt):
    from powdr_amd import air_text, prover
    from powdr_amd import system_airs as sa
    from powdr_amd.periphery import _col, _neg_col, _tables

    # the boundary AIR of before the keyword existed, built here from its definition: the three buses' tables laid end to end
    col = {n: i for i, n in enumerate(sa.BOUNDARY_COLUMNS)}
    rows = prover.row_operands(sa.BOUNDARY_WIDTH)
    bc, spans = [], []
    for _, text in sa.BOUNDARY_CONSTRAINTS:
        code = air_text.compile_expr(text, col, rows)
        spans.append((len(bc), len(code)))
        bc += code
    c, const, valid = (lambda n: _col(col[n])), (lambda v: [1, v]), _col(col["is_valid"])
    by_bus = [(1, [(valid, [c("as"), c("ptr")] + [c(f"init{i}") for i in range(4)] + [c("init_ts")]),
                   (_neg_col(col["is_valid"]), [c("as"), c("ptr")] + [c(f"fin{i}") for i in range(4)] + [c("fin_ts")])]),
              (3, [(valid, [c("p_lo"), const(17)]), (valid, [c("p_hi"), const(12)]), (valid, [c("d_lo"), const(17)]), (valid, [c("d_hi"), const(12)])]),
              (6, [(valid, [c("init0"), c("init1"), const(0), const(0)]), (valid, [c("init2"), c("init3"), const(0), const(0)])])]
    inter, ispans, ibc = [], [], []
    for bus, rows_ in by_bus:
        it, sp, code = _tables(bus, rows_)
        inter += [[b, n, f + len(ispans)] for b, n, f in it.tolist()]
        ispans += [[o + len(ibc), ln] for o, ln in sp.tolist()]
        ibc += code.tolist()
    before = [np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2), np.array(inter, np.uint32), np.array(ispans, np.uint32), np.array(ibc, np.uint32)]
    for air in (sa.boundary_air(), sa.boundary_air(leaf_bus=None)):
        now = [air.cons[0], air.cons[1], *air.inter]
        assert all(a.dtype == b.dtype and a.shape == b.shape and (a == b).all() for a, b in zip(before, now))
        assert air.width == 18 and air.columns == sa.BOUNDARY_COLUMNS and air.transition and air.n_public == 0
    # with a leaf bus: the same programs and one more interaction, nine arguments, of degree 1
    leaf = sa.boundary_air(leaf_bus=9)
    assert (leaf.cons[0] == before[0]).all() and (leaf.inter[0][:-1] == before[2]).all() and leaf.inter[0][-1].tolist() == [9, 9, len(before[3])]
    assert (leaf.inter[1][:len(before[3])] == before[3]).all() and (leaf.inter[2][:len(before[4])] == before[4]).all()
    assert leaf.columns == sa.BOUNDARY_COLUMNS and prover.public_programs_check(18, leaf.cons[0], leaf.cons[1], 0, leaf.inter)["max_degree"] <= 3
    for h in (0, 31, 40):
        with pytest.raises(ValueError):
            mt.merkle_air(h)
    assert mt.merkle_air(1).width == 55 and mt.merkle_air(30).width == 55
    with pytest.raises(ValueError):
        mt.merkle_air(30, merkle_bus=5)


def test_the_leaf_send_of_the_boundary_is_the_key_and_words_of_boundary_leaves():
    """boundary_air(leaf_bus=9) on a numpy boundary trace sends exactly what the stand-in of the tests sends for the same locations"""
    from powdr_amd import system_airs as sa
    from tests import _system_airs_ref as sref

    rng = np.random.default_rng(3)
    space = np.array([1, 1, 2, 2, 2])
    ptr = np.array([0, 4, 0, 8, (1 << 29) - 4])
    init, fin = rng.integers(0, 256, (4, 5)), rng.integers(0, 256, (4, 5))
    trace = sref.boundary_from_arrays(space, ptr, init, rng.integers(0, 99, 5), fin, 100 + rng.integers(0, 99, 5))
    keys = (space - 1) * (1 << 29) + ptr
    assert keys[-1] == (1 << 30) - 4
    stand_in = mref.leaf_sender(keys, init.T, fin.T)
    mine = mref.bm.tally([(list(trace.astype(np.int64)), sa.boundary_air(leaf_bus=9).inter)])[0]
    theirs = mref.bm.tally([stand_in])[0]
    assert {k: e[0] for k, e in mine.items() if k[0] == 9} == {k: e[0] for k, e in theirs.items()} and len(theirs) == 5


# ---- every leaf set at height 3 ---------------------------------------------------------------------------------------------------------
def test_every_leaf_set_at_height_3_satisfies_the_air_and_closes_the_buses(mt, constants):
    stored = [1, 2, 6]
    for r in range(1, 9):
        for keys in itertools.combinations(range(8), r):
            case = Case(mt, constants, 3, stored, keys, seed=r)
            assert case.violations() == {}, (keys, case.violations())  # (padding included: every row of the 2^log_height is evaluated)
            assert case.unbalanced() == set(), keys
            assert (case.public[:8] == case.root_before).all() and (case.public[8:] == case.root_after).all()
            n = len(case.where)
            assert case.cols[mref.VALID].sum() == n and not case.cols[:, n:].any() and case.cols[mref.IS_ROOT].tolist() == [1] + [0] * (case.cols.shape[1] - 1)
            assert case.cols[mref.IS_LEAF].sum() == r


# ---- tampering ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["height_3", "height_30"])
def case(request, mt, constants):
    if request.param == "height_3":
        return Case(mt, constants, 3, [1, 2, 6], [1, 4, 5], seed=21)
    c = Case(mt, constants, 30, [1, 77, (1 << 29) + 5, (1 << 30) - 1], EDGE_KEYS_30, seed=22)
    assert c.violations() == {} and c.unbalanced() == set()
    return c


def one_touched_child(case):
    """a row above the leaves with exactly one touched child -> (node, row, the untouched side: 0 left / 1 right)"""
    for node, r in sorted(case.where.items()):
        lt, rt = int(case.cols[mref.LEFT_TOUCHED, r]), int(case.cols[mref.RIGHT_TOUCHED, r])
        if node[0] >= 1 and lt + rt == 1:
            return node, r, 0 if rt else 1
    raise AssertionError("no such row")


def middle_row(case):
    """a row that is neither the root nor a leaf, whose parent has a row -> (node, row)"""
    node = next(n for n in sorted(case.where) if 1 <= n[0] < case.height)
    return node, case.where[node]


def test_1_every_cell_of_every_valid_row_raised_by_one(case):
    """Column c is raised on all valid rows at once and the catches are read per row. That is the same as raising one cell at a time:
    every constraint reads the cells of ONE row (the current one, or — `is_transition * is_root'` alone — the next one, so its
    violation on row r - 1 belongs to row r), and a row's bus tuples are functions of that row. The buses are compared row by row:
    the honest system is balanced, so a bus stays balanced exactly when the row's signed multiset of tuples on it did not change (the
    chip is the honest one: a chip remade for a changed pair receives that pair's true digest, which the row does not send either)."""
    cols, inter = case.cols, case.air.inter
    valid = np.nonzero(cols[mref.VALID])[0].tolist()
    honest = {r: mref.row_tuples(list(cols), r, inter) for r in valid}
    for c in range(mref.WIDTH):
        bad = cols.copy()
        bad[c, valid] = (bad[c, valid] + 1) % P
        by_row = {r: set() for r in valid}
        for name, rows in case.violations(bad).items():
            for r in rows:
                r = r + 1 if name == "no root after the first row" else r
                if r in by_row:
                    by_row[r].add(name)
        for r in valid:
            now = mref.row_tuples(list(bad), r, inter)
            buses = {k[0] for k in set(honest[r]) | set(now) if honest[r].get(k, 0) != now.get(k, 0)}
            root, leaf = bool(cols[mref.IS_ROOT, r]), bool(cols[mref.IS_LEAF, r])
            if c == mref.VALID:
                want = "valid boolean"
            elif c == mref.IS_ROOT:
                want = "is_root boolean" if root else "no root after the first row"
            elif c == mref.IS_LEAF:
                want = "is_leaf boolean" if leaf else "leaf level"
            elif c in (mref.LEFT_TOUCHED, mref.RIGHT_TOUCHED):
                side = "left" if c == mref.LEFT_TOUCHED else "right"
                want = f"{side}_touched boolean" if cols[c, r] else f"leaf {side} untouched" if leaf else mref.BUS_MERKLE
            elif c == mref.LEVEL:
                want = "root level" if root else "leaf level" if leaf else mref.BUS_MERKLE
            elif c == mref.INDEX:
                want = "root index" if root else mref.BUS_LEAF if leaf else mref.BUS_MERKLE
            else:
                want = mref.BUS_COMPRESS
            assert want in (buses if isinstance(want, int) else by_row[r]), (c, r, want, by_row[r], buses)
            if c >= mref.OUT0 and root and (c < mref.LEFT1 or c >= mref.OUT1):  # the root's digests are the public values
                assert f"root {'before' if c < mref.LEFT1 else 'after'} {(c - mref.OUT0) % 8}" in by_row[r]


def test_2_an_untouched_sibling_changed_in_phase_1_only(case):
    """...with out1 hashed again up to the root, the chip remade and even the public root moved along: every bus closes, and what is
    left is the constraint that an untouched child does not change"""
    node, r, side = one_touched_child(case)
    bad = case.cols.copy()
    c = (mref.LEFT1, mref.RIGHT1)[side] + 3
    bad[c, r] = (bad[c, r] + 1) % P
    new_root = mref.rehash_up(bad, case.where, node, 1, case.constants)
    public = np.concatenate([case.public[:8], new_root])
    names, buses = case.caught(bad, public)
    assert names == {f"untouched {('left', 'right')[side]} child 3"} and buses == set()
    # with the root the verifier expects, the root row objects too
    assert any(n.startswith("root after") for n in case.caught(bad)[0])


def test_3_a_middle_row_of_a_path_removed(case):
    node, r = middle_row(case)
    bad = case.cols.copy()
    bad[:, r] = 0
    names, buses = case.caught(bad)
    assert names == set() and buses == {mref.BUS_MERKLE}


def test_4_a_row_of_a_path_duplicated(mt, constants, case):
    # one more bit of height: there is a padding row to put the copy in
    wide = Case(mt, constants, case.height, case.stored, case.keys, case.seed, log_height=case.cols.shape[1].bit_length())
    assert (wide.cols[:, :case.cols.shape[1]] == case.cols).all() and wide.violations() == {} and wide.unbalanced() == set()
    node, r = middle_row(wide)
    bad = wide.cols.copy()
    free = len(wide.where)
    assert not bad[:, free].any()
    bad[:, free] = bad[:, r]
    names, buses = wide.caught(bad)
    assert names == set() and buses == {mref.BUS_MERKLE}
    leaf = wide.where[(0, wide.keys[0])]
    bad = wide.cols.copy()
    bad[:, free] = bad[:, leaf]
    assert wide.caught(bad) == (set(), {mref.BUS_MERKLE, mref.BUS_LEAF})


def test_5_left_and_right_swapped_on_one_row(case):
    node, r = middle_row(case)
    bad = case.cols.copy()
    for a, b in ((mref.LEFT0, mref.RIGHT0), (mref.LEFT1, mref.RIGHT1)):
        bad[a:a + 8, r], bad[b:b + 8, r] = case.cols[b:b + 8, r], case.cols[a:a + 8, r]
    bad[mref.LEFT_TOUCHED, r], bad[mref.RIGHT_TOUCHED, r] = case.cols[mref.RIGHT_TOUCHED, r], case.cols[mref.LEFT_TOUCHED, r]
    names, buses = case.caught(bad)
    assert {mref.BUS_COMPRESS, mref.BUS_MERKLE} <= buses  # the digests are not those of the swapped pair, and the children sit on the other side
    # hashed again up to the root, with the public roots moved along: the children's sends still name the side they are on
    for phase in (0, 1):
        root = mref.rehash_up(bad, case.where, node, phase, case.constants)
        public = root if phase == 0 else np.concatenate([public, root])
    names, buses = case.caught(bad, public)
    assert buses == {mref.BUS_MERKLE} and not any(n.startswith("root") for n in names)


def test_6_the_public_root_after_off_by_one(case):
    for k in (8, 15):
        public = case.public.copy()
        public[k] = (public[k] + 1) % P
        assert case.caught(case.cols, public) == ({f"root after {k - 8}"}, set())
    public = case.public.copy()
    public[2] = (public[2] + 1) % P
    assert case.caught(case.cols, public) == ({"root before 2"}, set())


def test_7_a_fin_word_changed_in_the_merkle_trace_but_not_in_the_boundary(case):
    """...hashed again up to the root, chip remade, public root moved along: the leaf bus is what is left"""
    key = case.keys[-1]
    bad = case.cols.copy()
    r = case.where[(0, key)]
    bad[mref.LEFT1 + 2, r] = (bad[mref.LEFT1 + 2, r] + 1) % P
    new_root = mref.rehash_up(bad, case.where, (0, key), 1, case.constants)
    assert case.caught(bad, np.concatenate([case.public[:8], new_root])) == (set(), {mref.BUS_LEAF})
    # the same for an init word
    bad = case.cols.copy()
    bad[mref.LEFT0 + 1, r] = (bad[mref.LEFT0 + 1, r] + 1) % P
    new_root = mref.rehash_up(bad, case.where, (0, key), 0, case.constants)
    assert case.caught(bad, np.concatenate([new_root, case.public[8:]])) == (set(), {mref.BUS_LEAF})


def test_8_a_second_root_row(case):
    node, r = middle_row(case)
    bad = case.cols.copy()
    bad[mref.IS_ROOT, r] = 1
    names, buses = case.caught(bad)
    assert "no root after the first row" in names and case.violations(bad)["no root after the first row"] == [r - 1]
    # a second root row that copies the first one entirely: still one row too many
    bad = case.cols.copy()
    bad[:, r] = bad[:, 0]
    assert "no root after the first row" in case.caught(bad)[0]
