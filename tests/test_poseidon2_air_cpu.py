"""The Poseidon2 compression chip (powdr_amd/system_airs.py poseidon2_air), no GPU: the numpy reference
(tests/_poseidon2_air_ref.py) is the library's permutation; the AIR has the shape the design states; its constraints vanish on reference
rows and pin every one of the 307 cells; with a hash user it balances the bus, and a wrong digest leaves exactly two tuples."""
import numpy as np
import pytest

from oracle import original_chips as ooc
from tests import _bus_multiset as bm
from tests import _poseidon2_air_ref as ref

P = ooc.P


@pytest.fixture
def second_table():
    from powdr_amd import prover

    rng = np.random.default_rng(0xC0FFEE)
    E, I = rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32)
    prover.set_poseidon2_constants(E, I)
    try:
        yield E, I
    finally:
        prover.set_poseidon2_constants()


@pytest.fixture(scope="module")
def chip():
    from powdr_amd import prover
    from powdr_amd import system_airs as sa

    constants = prover.poseidon2_constants()
    rng = np.random.default_rng(21)
    inputs = rng.integers(0, P, (11, 16), dtype=np.int64)  # 11 rows + 5 padding rows
    requests = [(w, 1 + (i % 3)) for i, w in enumerate(inputs.tolist())]
    trace, n = ref.compress_rows(requests, constants)
    assert n == 11 and trace.shape == (307, 16)
    return dict(air=sa.poseidon2_air(), constants=constants, inputs=inputs, trace=trace)


def _against_host(constants):
    from powdr_amd import prover

    rng = np.random.default_rng(8)
    inputs = np.concatenate([rng.integers(0, P, (64, 16), dtype=np.int64), np.zeros((1, 16), np.int64)])
    final, cells = ref.permute(inputs, constants)
    for k in range(len(inputs)):
        assert (final[k] == prover.poseidon2_host(inputs[k].astype(np.uint32))).all(), k
    assert (cells[ref.OUT:ref.OUT + 8].T == final[:, :8]).all()


def test_reference_is_the_host_permutation():
    from powdr_amd import prover

    _against_host(prover.poseidon2_constants())


def test_reference_is_the_host_permutation_under_a_second_table(second_table):
    from powdr_amd import prover

    e, i, _ = prover.poseidon2_constants()
    assert (e == second_table[0]).all() and (i == second_table[1]).all()
    _against_host(prover.poseidon2_constants())


def _walk(code):
    """(degree, maximal stack depth) of one post-fix program"""
    st, ip, deepest = [], 0, 0
    while ip < len(code):
        op = code[ip]
        if op in (0, 1):
            st.append(1 if op == 0 else 0)
            ip += 2
        elif op == 5:
            ip += 1
        else:
            y, x = st.pop(), st.pop()
            st.append(x + y if op == 4 else max(x, y))
            ip += 1
        deepest = max(deepest, len(st))
    assert len(st) == 1
    return st[0], deepest


def test_shape(chip):
    from powdr_amd import system_airs as sa

    air = chip["air"]
    assert air.width == 307 == sa.POSEIDON2_WIDTH == len(air.columns) == ref.WIDTH and air.pre_width == 0 and not air.transition and air.n_public == 0
    assert (sa.P2_IN, sa.P2_FULL, sa.P2_PARTIAL, sa.P2_OUT) == (ref.IN, ref.FULL, ref.PARTIAL, ref.OUT) and sa.BUS_COMPRESS == 5
    bc, spans = air.cons
    walks = [_walk(bc[o:o + n].tolist()) for o, n in np.asarray(spans).tolist()]
    degs = [d for d, _ in walks]
    assert len(degs) == 290 and degs.count(3) == 282 and degs.count(1) == 8 and degs[-8:] == [1] * 8
    assert max(depth for _, depth in walks) <= 8
    assert bc.max() < P and int(bc[np.nonzero(bc[:-1] == 0)[0] + 1].max()) <= 306  # (a loose look at the operands: constants are canonical)
    inter, ispans, ibc = air.inter
    assert inter.tolist() == [[5, 24, 0]] and len(ispans) == 25
    assert ibc.tolist() == [0, 0, 5] + [x for c in list(range(1, 17)) + list(range(299, 307)) for x in (0, c)]


def test_constraints_vanish_on_reference_rows(chip):
    t = chip["trace"]
    assert (t[0, 11:] == 0).all() and (t[1:17, 11:] == 0).all() and t[ref.OUT, 11:].all()  # padding: the zero input's honest row
    assert ooc.check_constraints(*chip["air"].cons, [t[c] for c in range(307)]) == (0, None)


def test_every_cell_is_pinned(chip):
    """row k of the experiment = reference row 3 with cell k raised by one: every one of the 307 changes is seen — by a constraint, or
    (mult, which no constraint reads) by the bus"""
    air, t = chip["air"], chip["trace"]
    rows = np.repeat(t[:, 3:4].astype(np.int64), 307, axis=1)
    rows[np.arange(307), np.arange(307)] = (rows[np.arange(307), np.arange(307)] + 1) % P
    cols = [rows[c] for c in range(307)]
    bc, spans = air.cons
    seen = np.zeros(307, bool)
    for o, n in np.asarray(spans).tolist():
        seen |= np.asarray(ooc.eval_postfix(bc[o:o + n], cols)) % P != 0
    assert seen[1:].all(), np.nonzero(~seen)[0]
    assert not seen[0]
    user = ref.hash_user_trace(chip["inputs"], chip["constants"], 4, valid=[1 + (i % 3) for i in range(11)])
    ui = ref.hash_user_interactions(5)
    assert not any(e[0] for e in bm.tally([(user, ui), (t, air.inter)])[0].values())
    bad = t.copy()
    bad[0, 3] += 1
    left = [(k, e) for k, e in bm.tally([(user, ui), (bad, air.inter)])[0].items() if e[0]]
    assert len(left) == 1 and left[0][0][2][:16] == tuple(chip["inputs"][3].tolist()) and left[0][1][0] == P - 1


def test_a_hash_user_balances_and_a_wrong_digest_leaves_two_tuples(chip):
    air, t = chip["air"], chip["trace"]
    user = ref.hash_user_trace(chip["inputs"], chip["constants"], 4, valid=[1 + (i % 3) for i in range(11)])
    ui = ref.hash_user_interactions(5)
    table, active = bm.tally([(user, ui), (t, air.inter)])
    assert active == {5: 22} and len(table) == 11 and not any(e[0] for e in table.values())
    user[17 + 2, 6] = (int(user[17 + 2, 6]) + 1) % P
    left = sorted((k, e) for k, e in bm.tally([(user, ui), (t, air.inter)])[0].items() if e[0])
    assert len(left) == 2 and all(k[2][:16] == tuple(chip["inputs"][6].tolist()) for k, _ in left)
    assert sorted(e[0] for _, e in left) == [1, P - 1] and {e[1][0] for _, e in left} == {0, 1}


def test_an_air_of_one_table_rejects_rows_of_another(chip, second_table):
    from powdr_amd import prover
    from powdr_amd import system_airs as sa

    other = prover.poseidon2_constants()
    trace2, _ = ref.compress_rows([(w, 1) for w in chip["inputs"].tolist()], other)
    cols2 = [trace2[c] for c in range(307)]
    assert ooc.check_constraints(*chip["air"].cons, cols2)[0] > 0
    assert ooc.check_constraints(*sa.poseidon2_air().cons, cols2) == (0, None)
    assert ooc.check_constraints(*sa.poseidon2_air().cons, [chip["trace"][c] for c in range(307)])[0] > 0


def test_rust_and_python_bind_the_new_entry():
    from powdr_amd import abi
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    assert c.get("pw_poseidon2_compress_trace") == 10 == r.get("pw_poseidon2_compress_trace")
    assert hasattr(abi.lib, "pw_poseidon2_compress_trace")
