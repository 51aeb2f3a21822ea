"""tests/_commit_ref.py (the numpy reference the commitment kernels are tested against, tests/test_commit_kernels_gpu.py) against the
oracle: the sponge and the binary tree against sm.merkle_commit, the mixed-height tree against the main root of sm.prove_segment, the
FRI leaves against sm.poseidon2 — under the placeholder constants and under one edge table. Exact arithmetic: every comparison is
equality."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _commit_ref as ref
from tests import _poseidon2_tables as tables

P = om.P
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))


def rows_of(flat, height, width):
    """column-major flat words -> [height, width]"""
    return np.ascontiguousarray(np.asarray(flat, np.uint32).reshape(width, height).T)


def check_binary(height, width, seed=0):
    k = sm.poseidon2_constants()
    m = np.random.default_rng(1000 * seed + 37 * height + width).integers(0, P, width * height, dtype=np.uint32)
    root, dig = sm.merkle_commit(m, height, width, want_digests=True)
    got = ref.binary_tree(ref.sponge(rows_of(m, height, width), k), k)
    assert got.shape == dig.shape and (got == dig).all()
    assert (got[-8:] == root).all()


@pytest.mark.parametrize("height,width", [(1, 1), (2, 7), (8, 8), (64, 9), (256, 17), (1024, 23)])
def test_sponge_and_binary_tree_equal_the_oracle_digests(height, width):
    check_binary(height, width)


def segment_airs(shapes, seed):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, P, w * (1 << lh), dtype=np.uint32), w, lh, *NO_CONS, None) for w, lh in shapes]


def check_mixed(shapes, seed):
    k = sm.poseidon2_constants()
    airs = segment_airs(shapes, seed)
    A = len(airs)
    want = sm.prove_segment(airs, num_queries=0, logup=False)[5 + 4 * A:5 + 4 * A + 8]  # the main root, right after the header
    mats = [rows_of(sm.lde(t, w, lh), 2 << lh, w) for t, w, lh, *_ in airs]
    got = ref.mixed_tree(mats, k)
    N = max(len(m) for m in mats)
    assert len(got) == (2 * N - 1) * 8
    assert (got[-8:] == want).all()


# two AIRs on one level and levels with none; a single AIR; one AIR on every level
@pytest.mark.parametrize("shapes", [[(5, 4), (3, 2), (9, 4), (2, 0)], [(11, 3)], [(1 + 3 * lh, lh) for lh in range(6)]], ids=["shared_level", "one_air", "every_level"])
def test_mixed_tree_root_equals_the_oracle_main_root(shapes):
    check_mixed(shapes, seed=len(shapes))


def test_a_mixed_tree_of_one_matrix_is_not_the_binary_tree():
    """the pairing differs (j, j + n against 2j, 2j + 1): the two builders agree on the leaves only — a reference that mixed them up
    would pass neither comparison above, and this keeps it that way"""
    k = sm.poseidon2_constants()
    m = np.random.default_rng(5).integers(0, P, (8, 3), dtype=np.uint32)
    a, b = ref.mixed_tree([m], k), ref.binary_tree(ref.sponge(m, k), k)
    assert (a[:64] == b[:64]).all() and (a[64:] != b[64:]).any()


def check_ext_pairs():
    k = sm.poseidon2_constants()
    v = np.random.default_rng(8).integers(0, P, (8, 4), dtype=np.uint32)
    v[0], v[5] = P - 1, 0
    got = ref.ext_pair_leaves(v, k)
    assert got.shape == (4, 8)
    for i in range(4):
        want = sm.poseidon2(np.concatenate([v[i], v[i + 4], np.zeros(8, np.uint32)]))[:8]
        assert (got[i] == want).all()


def test_ext_pair_leaves_equal_the_oracle_permutation():
    check_ext_pairs()


@pytest.mark.parametrize("name", ["plus_half", "minus_half", "random_0"])
def test_the_reference_follows_an_installed_edge_table(name):
    E, I = next((e, i) for n, _, e, i in tables.named_tables() if n == name)
    placeholder = sm.poseidon2_constants()
    try:
        sm.set_poseidon2_constants(E, I)
        k = sm.poseidon2_constants()
        assert (k[0] == E).all() and (k[1] == I).all() and (k[0] != placeholder[0]).any()
        check_binary(64, 9, seed=1)
        check_mixed([(5, 4), (3, 2), (9, 4), (2, 0)], seed=2)
        check_ext_pairs()
        for kind, m in tables.edge_matrices(16, 17).items():
            _, dig = sm.merkle_commit(m, 16, 17, want_digests=True)
            assert (ref.binary_tree(ref.sponge(rows_of(m, 16, 17), k), k) == dig).all(), kind
    finally:
        sm.set_poseidon2_constants()
    assert (sm.poseidon2_constants()[0] == placeholder[0]).all()
