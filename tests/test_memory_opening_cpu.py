"""Openings of the memory tree without a GPU (powdr_amd/memory_tree.py verify_opening, pw_memory_opening_verify): the
host verifier against the openings of tests/_memory_opening_ref.py — every key set at height 3, random sets at height 6 against the
dense brute-force root, the sibling counts — in agreement with the reference's numpy verifier, every way an opening can be wrong on
one height-3 and one height-30 case (20: another root; 19: malformed), a false non-membership claim, and the refusals of
pw_memory_tree_open that need no GPU. Every comparison is exact."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import _memory_opening_ref as oref
from tests import _memory_tree_ref as tref

P = tref.P


def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


@pytest.fixture(scope="module")
def mt():
    from powdr_amd import memory_tree

    return memory_tree


def tree_with(height, stored, seed):
    rng = np.random.default_rng(seed)
    t = tref.SparseTree(height, constants())
    t.write(stored, rng.integers(0, P, (len(stored), 8), dtype=np.uint32))
    return t


def test_every_key_set_at_height_3(mt):
    t = tree_with(3, [1, 2, 6], 1)
    k = constants()
    for r in range(1, 9):
        for keys in itertools.combinations(range(8), r):
            pay, sib = oref.opening(t, keys)
            assert len(sib) == oref.sibling_count(3, keys) <= r * 3
            assert mt.verify_opening(3, t.root(), keys, pay, sib) == (0, 0), keys
            assert oref.verify(3, t.root(), keys, pay, sib, k) == 0, keys
            for j, key in enumerate(keys):
                assert (pay[j] == t.payload.get(key, np.zeros(8, np.uint32))).all()


def test_random_sets_at_height_6_against_the_dense_root(mt):
    k = constants()
    rng = np.random.default_rng(2)
    for trial in range(12):
        stored = np.sort(rng.choice(64, int(rng.integers(1, 40)), replace=False))
        t = tree_with(6, stored.tolist(), 100 + trial)
        root = tref.dense_root(6, t.payload, k)
        keys = np.sort(rng.choice(64, int(rng.integers(1, 30)), replace=False))
        pay, sib = oref.opening(t, keys)
        assert mt.verify_opening(6, root, keys, pay, sib) == (0, 0), trial
        assert oref.verify(6, root, keys, pay, sib, k) == 0


@pytest.mark.parametrize("height", [1, 3, 30, 40])
def test_the_sibling_counts(mt, height):
    t = tree_with(height, [0, (1 << height) - 1], height)
    last = (1 << height) - 1
    for keys, want in (([0], height), ([last], height), ([0, 1], height - 1)):
        pay, sib = oref.opening(t, keys)
        assert len(sib) == want and mt.verify_opening(height, t.root(), keys, pay, sib) == (0, 0)
    if height <= 3:
        keys = list(range(1 << height))
        pay, sib = oref.opening(t, keys)
        assert sib.shape == (0, 8) and mt.verify_opening(height, t.root(), keys, pay, sib) == (0, 0)


CASES = {3: ([1, 2, 6, 7], [0, 1, 4, 7]), 30: ([1, 77, (1 << 29) + 5, (1 << 30) - 1], [0, 1, 1 << 29, (1 << 30) - 1])}


@pytest.mark.parametrize("height", sorted(CASES))
def test_every_way_an_opening_can_be_wrong(mt, height):
    stored, keys = CASES[height]
    k = constants()
    t = tree_with(height, stored, 7 + height)
    root = t.root().copy()
    keys = np.array(keys, np.uint64)
    pay, sib = oref.opening(t, keys)
    n, m = len(keys), len(sib)
    assert pay[0].any() == (0 in stored) and pay[1].any() and not pay[2].any() and pay[3].any()  # stored and absent leaves
    both = lambda *a: (mt.verify_opening(height, *a)[0], oref.verify(height, *a, k))
    assert both(root, keys, pay, sib) == (0, 0)
    # 20: the opening hashes to another root
    for i in range(8 * n):
        bad = pay.copy()
        bad.reshape(-1)[i] = (int(bad.reshape(-1)[i]) + 1) % P
        assert mt.verify_opening(height, root, keys, bad, sib)[0] == 20, i
    for i in range(8 * m):
        bad = sib.copy()
        bad.reshape(-1)[i] = (int(bad.reshape(-1)[i]) + 1) % P
        assert mt.verify_opening(height, root, keys, pay, bad)[0] == 20, i
    assert both(root, keys, (pay + (np.arange(8 * n).reshape(n, 8) == 9)) % P, sib) == (20, 20)
    for i in range(8):
        bad = root.copy()
        bad[i] = (int(bad[i]) + 1) % P
        assert both(bad, keys, pay, sib) == (20, 20)
    swaps = [(a, b) for a, b in ((0, 1), (0, m - 1), (m // 2, m // 2 + 1), (m - 2, m - 1)) if (sib[a] != sib[b]).any()]
    assert len(swaps) >= 2  # (two equal siblings — the Z_0 next to two lone absent leaves — swapped are the same opening)
    for a, b in swaps:
        bad = sib.copy()
        bad[[a, b]] = bad[[b, a]]
        assert both(root, keys, pay, bad) == (20, 20)
    moved = keys.copy()
    moved[3] ^= np.uint64(1)  # a stored leaf's payload claimed for its neighbour: as many siblings, at the same places
    assert oref.sibling_count(height, moved) == m and both(root, moved, pay, sib) == (20, 20)
    # ... a stored leaf claimed absent
    absent = pay.copy()
    absent[3] = 0
    assert both(root, keys, absent, sib) == (20, 20)
    # 19: malformed; the count the keys imply comes back where no key or word is at fault
    assert mt.verify_opening(height, root, keys, pay, sib[:-1]) == (19, m) and oref.verify(height, root, keys, pay, sib[:-1], k) == 19
    more = np.concatenate([sib, sib[:1]])
    assert mt.verify_opening(height, root, keys, pay, more) == (19, m) and oref.verify(height, root, keys, pay, more, k) == 19
    swapped = keys[[0, 2, 1, 3]]
    assert mt.verify_opening(height, root, swapped, pay, sib) == (19, 2) and oref.verify(height, root, swapped, pay, sib, k) == 19
    twice = keys[[0, 1, 1, 3]]
    assert mt.verify_opening(height, root, twice, pay, sib) == (19, 2)
    beyond = keys.copy()
    beyond[3] = np.uint64(1 << height)
    assert mt.verify_opening(height, root, beyond, pay, sib) == (19, 3) and oref.verify(height, root, beyond, pay, sib, k) == 19
    for name, arr, at in (("root", root, 5), ("pay", pay, 8 * n - 1), ("sib", sib, 8 * m - 3)):
        for word in (P, 0xFFFFFFFF):
            bad = arr.copy()
            bad.reshape(-1)[at] = word
            args = dict(root=root, pay=pay, sib=sib)
            args[name] = bad
            assert mt.verify_opening(height, args["root"], keys, args["pay"], args["sib"]) == (19, at), name
            assert oref.verify(height, args["root"], keys, args["pay"], args["sib"], k) == 19
    none = np.zeros(0, np.uint64)
    assert mt.verify_opening(height, root, none, np.zeros((0, 8), np.uint32), sib)[0] == 19
    for h in (0, 41):
        assert mt.verify_opening(h, root, keys, pay, sib)[0] == 19


def test_a_stored_leaf_opened_with_the_zero_payload_fails(mt):
    """a false non-membership claim: the one stored leaf, alone and next to its absent sibling"""
    for height in (3, 30):
        key = (1 << height) - 2
        t = tree_with(height, [key], 21)
        for keys in ([key], [key, key + 1]):
            pay, sib = oref.opening(t, keys)
            assert pay[0].any() and mt.verify_opening(height, t.root(), keys, pay, sib) == (0, 0)
            assert mt.verify_opening(height, t.root(), keys, np.zeros_like(pay), sib)[0] == 20
            # and the reverse: a payload claimed for the absent sibling
            if len(keys) == 2:
                assert not pay[1].any() and mt.verify_opening(height, t.root(), keys, pay[[0, 0]], sib)[0] == 20
        # an empty tree holds nothing anywhere
        empty = tref.SparseTree(height, constants())
        pay0, sib0 = oref.opening(empty, [key])
        assert not pay0.any() and mt.verify_opening(height, empty.root(), [key], pay0, sib0) == (0, 0)
        assert mt.verify_opening(height, empty.root(), [key], pay[:1], sib0)[0] == 20


def test_the_verifier_is_tied_to_the_installed_table(mt):
    from powdr_amd import prover

    t = tree_with(6, [3, 40], 5)
    pay, sib = oref.opening(t, [3, 9])
    assert mt.verify_opening(6, t.root(), [3, 9], pay, sib) == (0, 0)
    rng = np.random.default_rng(0xC0FFEE)
    prover.set_poseidon2_constants(rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32))
    try:
        assert mt.verify_opening(6, t.root(), [3, 9], pay, sib)[0] == 20
    finally:
        prover.set_poseidon2_constants()
    assert mt.verify_opening(6, t.root(), [3, 9], pay, sib) == (0, 0)


def test_open_refuses_null_pointers_and_no_keys_before_any_gpu_call(mt):
    from powdr_amd import prover

    t = mt.MemoryTree(30)
    keys, pay, sib = np.array([5], np.uint64), np.full(8, 0x5A5A5A5A, np.uint32), np.full(8 * 30, 0x5A5A5A5A, np.uint32)
    m, status, info = C.c_uint64(77), C.c_uint32(77), C.c_uint64(77)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [t._h, ptr(keys), 1, ptr(pay), ptr(sib), 30, C.byref(m), C.byref(status), C.byref(info)]
    f = mt.lib.pw_memory_tree_open
    for at in (0, 1, 3, 4, 6, 7, 8):
        args = list(good)
        args[at] = None
        assert f(*args) == -1, at
    args = list(good)
    args[2] = 0
    assert f(*args) == -1
    rng = np.random.default_rng(0xC0FFEE)
    prover.set_poseidon2_constants(rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32))
    try:
        assert f(*good) == -1  # the installed table is not the tree's
    finally:
        prover.set_poseidon2_constants()
    assert (m.value, status.value, info.value) == (77, 77, 77) and (pay == 0x5A5A5A5A).all() and (sib == 0x5A5A5A5A).all()
    assert t.stats() == dict(leaves=0, stored_nodes=0, device_bytes=0, last_permutations=0, last_launches=0, last_scratch_bytes=0)
    t.close()


def test_the_symbols_load_and_are_bound_in_rust(mt):
    from powdr_amd import abi, prover
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name, arity in (("pw_memory_tree_open", 9), ("pw_memory_opening_verify", 8)):
        assert hasattr(abi.lib, name) and name in prover.PROVER_SYMBOLS
        assert c.get(name) == arity == r.get(name), name
    assert set(mt.OPEN_STATUS) == {0, 1, 4}
