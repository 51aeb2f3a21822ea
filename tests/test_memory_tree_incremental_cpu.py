"""The mode of a memory tree without a GPU (pw_memory_tree_set_mode / pw_memory_tree_get_mode, powdr_amd/memory_tree.py):
the default, the refusals, that the mode changes nothing an empty tree answers, the Python property, the table tie, the symbols."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import _memory_tree_ref as ref

P = ref.P
EMPTY_STATS = dict(leaves=0, stored_nodes=0, device_bytes=0, last_permutations=0, last_launches=0, last_scratch_bytes=0)


def get_mode(mt, handle):
    mode = C.c_uint32(99)
    rc = mt.lib.pw_memory_tree_get_mode(handle, C.byref(mode))
    return rc, mode.value


def test_a_fresh_tree_is_in_rebuild_mode_and_the_mode_is_set_and_refused():
    from powdr_amd import memory_tree as mt

    assert (mt.MODE_REBUILD, mt.MODE_INCREMENTAL) == (0, 1)
    t = mt.MemoryTree(30)
    assert get_mode(mt, t._h) == (0, 0) and t.incremental is False
    assert mt.lib.pw_memory_tree_set_mode(t._h, 1) == 0 and get_mode(mt, t._h) == (0, 1) and t.incremental is True
    assert mt.lib.pw_memory_tree_set_mode(t._h, 7) == -1 and get_mode(mt, t._h) == (0, 1)  # an unknown mode: refused, the mode stays
    assert mt.lib.pw_memory_tree_set_mode(t._h, 2) == -1
    assert mt.lib.pw_memory_tree_set_mode(t._h, 0) == 0 and get_mode(mt, t._h) == (0, 0)
    assert mt.lib.pw_memory_tree_set_mode(None, 1) == -1 and get_mode(mt, None) == (-1, 99)
    assert mt.lib.pw_memory_tree_get_mode(t._h, None) == -1
    t.close()


@pytest.mark.parametrize("height", [1, 30, 40])
def test_the_empty_trees_root_and_stats_do_not_depend_on_the_mode(height):
    from powdr_amd import memory_tree as mt
    from powdr_amd import prover

    want = ref.zero_digests(height, prover.poseidon2_constants())[height]
    t = mt.MemoryTree(height)
    for on in (False, True, False):
        t.incremental = on
        assert t.incremental is on and (t.root() == want).all() and t.stats() == EMPTY_STATS
    t.close()


def test_the_constructor_argument_and_the_property():
    from powdr_amd import abi
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(3, incremental=True)
    assert t.incremental is True and t.height == 3
    t.incremental = False
    assert t.incremental is False
    t.close()
    assert mt.MemoryTree(3).incremental is False and mt.MemoryTree().height == 30
    with pytest.raises(abi.HipError):
        t.incremental = True  # a closed tree: the NULL handle


def test_both_calls_answer_minus_one_under_another_table_and_again_under_its_own():
    from powdr_amd import prover
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(30, incremental=True)
    rng = np.random.default_rng(0xC0FFEE)
    E, I = rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32)
    prover.set_poseidon2_constants(E, I)
    try:
        assert mt.lib.pw_memory_tree_set_mode(t._h, 0) == -1 and mt.lib.pw_memory_tree_set_mode(t._h, 1) == -1
        assert get_mode(mt, t._h) == (-1, 99)
    finally:
        prover.set_poseidon2_constants()
    assert get_mode(mt, t._h) == (0, 1)  # the refused set_mode(0) changed nothing
    t.close()


def test_the_symbols_load_and_are_bound_in_rust():
    from powdr_amd import abi, prover
    from tests.test_rust_adapter_sync import c_functions, rust_functions

    c, r = c_functions(), rust_functions()
    for name in ("pw_memory_tree_set_mode", "pw_memory_tree_get_mode"):
        assert hasattr(abi.lib, name) and name in prover.PROVER_SYMBOLS
        assert c.get(name) == 2 == r.get(name), name
    header = (Path(__file__).resolve().parents[1] / "include" / "powdr_prover.h").read_text()
    assert "#define PW_MEMORY_TREE_REBUILD 0u" in header and "#define PW_MEMORY_TREE_INCREMENTAL 1u" in header
