"""The sparse memory Merkle tree without a GPU (powdr_amd/memory_tree.py): the sparse numpy reference of
tests/_memory_tree_ref.py against a dense brute-force tree, the library's empty roots against the reference's Z_H under both constant
tables, the refusals of pw_memory_tree_create, the symbols, and a tree that answers -1 under another table than its own."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import _memory_tree_ref as ref

P = ref.P


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


def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


def test_the_sparse_reference_equals_the_dense_tree_for_every_leaf_set_at_height_3():
    k = constants()
    rng = np.random.default_rng(1)
    payloads = rng.integers(0, P, (8, 8), dtype=np.uint32)
    assert (ref.SparseTree(3, k).root() == ref.dense_root(3, {}, k)).all()
    for r in range(1, 9):
        for keys in itertools.combinations(range(8), r):
            t = ref.SparseTree(3, k)
            t.write(keys, payloads[list(keys)])
            assert (t.root() == ref.dense_root(3, {i: payloads[i] for i in keys}, k)).all(), keys


def test_the_sparse_reference_equals_the_dense_tree_for_random_sets_at_height_6():
    k = constants()
    rng = np.random.default_rng(2)
    for trial in range(12):
        n = int(rng.integers(1, 40))
        keys = np.sort(rng.choice(64, n, replace=False))
        payloads = rng.integers(0, P, (n, 8), dtype=np.uint32)
        t = ref.SparseTree(6, k)
        half = n // 2  # written in two steps, the second rewriting one leaf of the first
        t.write(keys[:half], payloads[:half])
        t.write(keys[max(half - 1, 0):], payloads[max(half - 1, 0):])
        assert (t.root() == ref.dense_root(6, dict(zip(keys.tolist(), payloads)), k)).all(), trial
        # the record rows of a further update end with the roots before and after it, and are compressions
        init = payloads[:3].copy()
        fin = rng.integers(0, P, (min(n, 3), 8), dtype=np.uint32)
        before = t.root().copy()
        m, ids, log_h, rows = t.update(keys[:3], init, fin)
        assert rows == len(ids) and (m[17:, rows // 2 - 1] == before).all() and (m[17:, rows - 1] == t.root()).all()
        assert (ref.compress(m[1:17, :rows].T, k) == m[17:, :rows].T).all()


@pytest.mark.parametrize("height", [1, 30, 40])
def test_the_empty_trees_root_is_z_h(height):
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(height)
    assert (t.root() == ref.zero_digests(height, constants())[height]).all()
    assert t.stats() == dict(leaves=0, stored_nodes=0, device_bytes=0, last_permutations=0, last_launches=0, last_scratch_bytes=0)
    t.close()


@pytest.mark.parametrize("height", [1, 30, 40])
def test_the_empty_trees_root_is_z_h_under_a_second_table(second_table, height):
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(height)
    want = ref.zero_digests(height, constants())[height]
    assert (constants()[0] == second_table[0]).all() and (t.root() == want).all()
    t.close()


def test_create_refuses_heights_outside_1_to_40():
    from powdr_amd import memory_tree as mt

    for h in (0, 41):
        assert not mt.lib.pw_memory_tree_create(h)
        with pytest.raises(ValueError):
            mt.MemoryTree(h)


def test_the_symbols_load_and_are_bound_in_rust():
    from powdr_amd import abi, prover
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name, arity in (("pw_memory_tree_create", 1), ("pw_memory_tree_destroy", 1), ("pw_memory_tree_root", 2), ("pw_memory_tree_stats", 2),
                        ("pw_memory_tree_update", 12), ("pw_memory_tree_boundary_leaves", 6)):
        assert hasattr(abi.lib, name) and name in prover.PROVER_SYMBOLS
        assert c.get(name) == arity == r.get(name), name


def test_a_tree_answers_minus_one_under_another_table_and_again_under_its_own():
    from powdr_amd import abi, prover
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(30)
    root = t.root()
    rng = np.random.default_rng(0xC0FFEE)
    E, I = rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32)
    prover.set_poseidon2_constants(E, I)
    try:
        out = np.zeros(8, np.uint32)
        st = mt.PwMemoryTreeStats()
        status, info = C.c_uint32(), C.c_uint64()
        assert mt.lib.pw_memory_tree_root(t._h, out.ctypes.data_as(C.c_void_p)) == -1 and not out.any()
        assert mt.lib.pw_memory_tree_stats(t._h, C.byref(st)) == -1
        assert mt.lib.pw_memory_tree_update(t._h, None, None, None, 0, None, None, 0, None, None, C.byref(status), C.byref(info)) == -1
        with pytest.raises(abi.HipError):
            t.root()
        other = mt.MemoryTree(30)  # a tree of the second table: another root
        assert (other.root() != root).any()
        other.close()
    finally:
        prover.set_poseidon2_constants()
    assert (t.root() == root).all()
    t.close()
