"""Openings of the memory tree on the device (powdr_amd/memory_tree.py MemoryTree.open, pw_memory_tree_open) against the
per-node reference of tests/_memory_opening_ref.py: payloads, siblings and their number word for word, verify_opening against the
tree's root, two runs the same bytes, the tree untouched by every call, the statuses against sentinel-filled buffers, and the outputs
of the three chained segments of tests/test_memory_merkle_gpu.py read out of the LAST proof's statement. Every comparison is exact.
The sizes are the smallest at which each path is taken: one workgroup is 256 keys, a level of at most TAIL_NODES nodes lives in the
tree's tail block, and the wrapper's first buffer holds max(1024, 4 n) siblings (the scattered sets need the retry)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _memory_opening_ref as oref
from tests import _memory_tree_ref as tref
from tests.test_memory_merkle_gpu import closed_with, execution, leaf_words, segment_of, statement  # noqa: F401 (execution: a fixture)
from tests.test_memory_tree_gpu import CUTS, TAIL_NODES, leaf_of, random_keys

pytestmark = pytest.mark.gpu
P = om.P
H = 30
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import prover

    return torch, prover


def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


def state_of(tree):
    s = tree.stats()
    return tree.root().tobytes(), s["leaves"], s["stored_nodes"], s["device_bytes"], tree.incremental


def checked_open(mt, tree, want, keys):
    """one opening on the device tree against the reference's of `want`: every word and the count; it verifies against the tree's
    root; a second run gives the same bytes; the tree is what it was -> (payloads, siblings)"""
    keys = np.asarray(keys, np.uint64)
    before = state_of(tree)
    status, info, pay, sib = tree.open(keys)
    assert (status, info) == (0, 0)
    want_pay, want_sib = oref.opening(want, keys)
    assert pay.shape == want_pay.shape and (pay == want_pay).all(), np.argwhere(pay != want_pay)[:5]
    assert sib.shape == want_sib.shape and (sib == want_sib).all(), np.argwhere(sib != want_sib)[:5]
    assert len(sib) <= len(keys) * tree.height
    assert (tree.root() == want.root()).all() and mt.verify_opening(tree.height, tree.root(), keys, pay, sib) == (0, 0)
    again = tree.open(keys, cap_siblings=len(sib))
    assert again[:2] == (0, 0) and again[2].tobytes() == pay.tobytes() and again[3].tobytes() == sib.tobytes()
    assert state_of(tree) == before
    return pay, sib


def test_every_key_set_at_height_3(gpu):
    from powdr_amd import memory_tree as mt

    stored = [1, 2, 6]
    pay = leaf_words(np.random.default_rng(1), 3, P)
    t, want = mt.MemoryTree(3), tref.SparseTree(3, constants())
    assert t.load(stored, pay) == (0, 0)
    want.write(stored, pay)
    for r in range(1, 9):
        for keys in itertools.combinations(range(8), r):
            checked_open(mt, t, want, keys)
    assert checked_open(mt, t, want, range(8))[1].shape == (0, 8) and len(checked_open(mt, t, want, [0, 1])[1]) == 2
    t.close()


@pytest.fixture(scope="module")
def loaded():
    """4096 scattered leaves at height 30 -> (keys, payloads, the reference tree): shared, never written"""
    keys0 = random_keys(8, 1 << 12)
    pay0 = np.random.default_rng(31).integers(0, P, (1 << 12, 8), dtype=np.uint32)
    want = tref.SparseTree(H, constants())
    want.write(keys0, pay0)
    return keys0, pay0, want


def key_sets(keys0):
    rng = np.random.default_rng(32)
    fresh = np.setdiff1d(random_keys(33, 400), keys0)
    scattered = np.unique(np.concatenate([rng.choice(keys0, 700, replace=False), fresh[:325]]))
    assert len(scattered) == TAIL_NODES + 1
    beside = np.setdiff1d(keys0[:40] ^ np.uint64(1), keys0)  # the siblings of stored leaves, not stored themselves
    assert len(beside) >= 30
    return {
        "edge_keys": np.array([0, 1, 1 << 29, (1 << 30) - 1], np.uint64),
        "one_stored_key": keys0[1234:1235],
        "consecutive_257": 1000 + np.arange(257, dtype=np.uint64),                      # more than one workgroup
        "scattered_1025": scattered,                                                    # T_0 and a few T_l above the tail threshold
        "every_stored_leaf": keys0,
        "keys_that_are_not_stored": np.unique(np.concatenate([beside, fresh[325:375]])),
        "a_stored_leaf_and_its_absent_sibling": np.unique(np.concatenate([keys0[:40], beside])),
    }


@pytest.fixture(scope="module")
def loaded_tree(gpu, loaded):
    from powdr_amd import memory_tree as mt

    t = mt.MemoryTree(H)
    assert t.load(loaded[0], loaded[1]) == (0, 0)
    yield t
    t.close()


@pytest.mark.parametrize("name", ["edge_keys", "one_stored_key", "consecutive_257", "scattered_1025", "every_stored_leaf", "keys_that_are_not_stored",
                                  "a_stored_leaf_and_its_absent_sibling"])
def test_height_30(gpu, loaded, loaded_tree, name):
    from powdr_amd import memory_tree as mt

    keys0, pay0, want = loaded
    keys = key_sets(keys0)[name]
    pay, sib = checked_open(mt, loaded_tree, want, keys)
    if name == "one_stored_key":
        assert len(sib) == H and (pay[0] == pay0[1234]).all()
    if name == "every_stored_leaf":
        assert (pay == pay0).all()
    if name == "keys_that_are_not_stored":
        assert not pay.any()
    if name == "scattered_1025":
        assert len(sib) > max(1024, 4 * len(keys))  # the wrapper's first buffer was too small: status 1 and the retry
    if name == "edge_keys":
        # 0 and 1 are each other's siblings; then three nodes a level, which pair up below the root: 2 + 3 * 27 + 1 + 0
        assert len(sib) == oref.sibling_count(H, keys) == 84


def test_after_an_update_in_both_modes(gpu, loaded):
    """the tree after an update that crosses the tail threshold, incremental and rebuilt: the same openings, byte for byte"""
    import copy

    from powdr_amd import memory_tree as mt

    keys0, pay0, want = loaded[0], loaded[1], copy.deepcopy(loaded[2])
    sets = key_sets(keys0)
    keys = sets["scattered_1025"]
    init = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)
    fin = np.random.default_rng(35).integers(0, P, (len(keys), 8), dtype=np.uint32)
    want.write(keys, fin)
    got = []
    for incremental in (True, False):
        t = mt.MemoryTree(H, incremental=incremental)
        assert t.load(keys0, pay0) == (0, 0)
        assert t.update(keys, init, fin, records=False)[:2] == (0, 0)
        got.append([checked_open(mt, t, want, sets[name]) for name in ("scattered_1025", "edge_keys", "a_stored_leaf_and_its_absent_sibling")])
        assert t.incremental == incremental
        t.close()
    for a, b in zip(*got):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert (got[0][0][0] == fin).all()


def test_a_tree_that_lives_in_the_tail_block(gpu):
    from powdr_amd import memory_tree as mt

    keys0 = random_keys(4, 1000)
    assert len(keys0) <= TAIL_NODES  # every level above the leaves is in the tail block
    pay0 = np.random.default_rng(36).integers(0, P, (1000, 8), dtype=np.uint32)
    t, want = mt.MemoryTree(H), tref.SparseTree(H, constants())
    assert t.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)
    checked_open(mt, t, want, keys0)
    checked_open(mt, t, want, np.unique(np.concatenate([keys0[::7], keys0[::5] ^ np.uint64(1), random_keys(37, 300)])))
    checked_open(mt, t, want, [int(keys0[500])])
    t.close()


@pytest.mark.parametrize("height", [1, 30])
def test_the_empty_tree(gpu, height):
    from powdr_amd import memory_tree as mt

    t, want = mt.MemoryTree(height), tref.SparseTree(height, constants())
    assert t.stats()["device_bytes"] == 0
    last = (1 << height) - 1
    for keys in ([0], [last], [0, last], sorted({0, 1, last >> 1, last})):
        status, info, pay, sib = t.open(keys)
        assert (status, info) == (0, 0) and not pay.any()
        assert t.stats()["device_bytes"] == (height + 1) * 32 and t.stats()["stored_nodes"] == 0  # Z_0 .. Z_H went to the device, no more
        checked_open(mt, t, want, keys)
    zero = tref.zero_digests(height, constants())
    assert (t.open([0])[3] == np.array(zero[:height])).all()
    # the tree still takes an update
    assert t.update([0], np.zeros((1, 8), np.uint32), np.ones((1, 8), np.uint32), records=False)[:2] == (0, 0)
    want.write([0], np.ones((1, 8), np.uint32))
    checked_open(mt, t, want, [0, last])
    t.close()


def test_height_40_with_keys_above_2_to_the_32(gpu):
    from powdr_amd import memory_tree as mt

    stored = np.array([3, (1 << 32) + 6, (1 << 39) + 1, (1 << 40) - 1], np.uint64)
    pay0 = np.random.default_rng(38).integers(0, P, (4, 8), dtype=np.uint32)
    t, want = mt.MemoryTree(40), tref.SparseTree(40, constants())
    assert t.load(stored, pay0) == (0, 0)
    want.write(stored, pay0)
    pay, sib = checked_open(mt, t, want, [2, (1 << 32) + 6, (1 << 32) + 7, 1 << 39, (1 << 40) - 1])
    assert (pay[1] == pay0[1]).all() and not pay[2].any() and (pay[4] == pay0[3]).all()
    assert len(checked_open(mt, t, want, [(1 << 40) - 1])[1]) == 40
    t.close()


def test_statuses_against_sentinel_filled_buffers(gpu, loaded):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    keys0, pay0, want = loaded
    t = mt.MemoryTree(H)
    assert t.load(keys0, pay0) == (0, 0)
    before = state_of(t)
    keys = key_sets(keys0)["consecutive_257"]
    n = len(keys)
    m = oref.sibling_count(H, keys)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()
    fresh = lambda rows: torch.full((rows, 8), SENTINEL, dtype=torch.int32, device="cuda")
    untouched = lambda *bufs: all(bool((b == SENTINEL).all()) for b in bufs)

    def call(k, cap, n_keys=None):
        pay, sib = fresh(n), fresh(m)
        got, status, info = C.c_uint64(77), C.c_uint32(77), C.c_uint64(77)
        torch.cuda.synchronize()
        rc = mt.lib.pw_memory_tree_open(t._h, k.data_ptr(), n if n_keys is None else n_keys, pay.data_ptr(), sib.data_ptr(), cap, C.byref(got), C.byref(status),
                                        C.byref(info))
        torch.cuda.synchronize()
        assert state_of(t) == before
        return rc, status.value, info.value, got.value, pay, sib

    # 0: written, and exactly m rows of them
    rc, status, info, got, pay, sib = call(dev(keys), m)
    assert (rc, status, info, got) == (0, 0, 0, m) and not untouched(pay) and not bool((sib == SENTINEL).all(dim=1).any())
    # 1: one row short: the count comes back, nothing is written; the wrapper hands the status on when the caller set the size
    rc, status, info, got, pay, sib = call(dev(keys), m - 1)
    assert (rc, status, info, got) == (0, 1, 0, m) and untouched(pay, sib)
    assert call(dev(keys), 0)[1:4] == (1, 0, m)
    assert t.open(keys, cap_siblings=m - 1) == (1, 0, None, None)
    # 4: the first key that is not above its predecessor, or not below 2^H
    for bad, at in ((keys[::-1], 1), (np.concatenate([keys[:100], keys[99:-1]]), 100), (np.concatenate([keys[:-1], [np.uint64(1 << H)]]), n - 1),
                    (np.concatenate([[np.uint64(1 << 63)], keys[1:]]), 0)):
        rc, status, info, got, pay, sib = call(dev(bad), m)
        assert (rc, status, info) == (0, 4, at) and untouched(pay, sib)
        assert t.open(bad) == (4, at, None, None)
    # -1 before any GPU call
    k = dev(keys)
    assert call(k, m, n_keys=0)[0] == -1
    got, status, info = C.c_uint64(77), C.c_uint32(77), C.c_uint64(77)
    pay, sib = fresh(n), fresh(m)
    f = mt.lib.pw_memory_tree_open
    assert f(None, k.data_ptr(), n, pay.data_ptr(), sib.data_ptr(), m, C.byref(got), C.byref(status), C.byref(info)) == -1
    assert f(t._h, None, n, pay.data_ptr(), sib.data_ptr(), m, C.byref(got), C.byref(status), C.byref(info)) == -1
    assert f(t._h, k.data_ptr(), n, None, sib.data_ptr(), m, C.byref(got), C.byref(status), C.byref(info)) == -1
    assert f(t._h, k.data_ptr(), n, pay.data_ptr(), None, m, C.byref(got), C.byref(status), C.byref(info)) == -1
    assert f(t._h, k.data_ptr(), n, pay.data_ptr(), sib.data_ptr(), m, None, C.byref(status), C.byref(info)) == -1
    rng = np.random.default_rng(0xC0FFEE)
    prover.set_poseidon2_constants(rng.integers(0, P, (8, 16), dtype=np.uint32), rng.integers(0, P, 13, dtype=np.uint32))
    try:
        assert f(t._h, k.data_ptr(), n, pay.data_ptr(), sib.data_ptr(), m, C.byref(got), C.byref(status), C.byref(info)) == -1
    finally:
        prover.set_poseidon2_constants()
    torch.cuda.synchronize()
    assert untouched(pay, sib) and (got.value, status.value, info.value) == (77, 77, 77) and state_of(t) == before
    # after all of them a correct update succeeds, and the tree opens as the reference does
    import copy

    want = copy.deepcopy(want)
    fin = np.random.default_rng(39).integers(0, P, (n, 8), dtype=np.uint32)
    init = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)
    assert t.update(keys, init, fin, records=False)[:2] == (0, 0)
    want.write(keys, fin)
    assert (checked_open(mt, t, want, keys)[0] == fin).all()
    t.close()


def test_the_outputs_of_three_chained_segments(gpu, execution, monkeypatch):
    """What a chain's statement says about the memory, read by a verifier that holds the proofs and two openings: the executor's final
    address-space-2 words against root_after of the LAST proof, the initial image against root_before of the first."""
    torch, prover = gpu
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa
    from tests import test_system_airs_gpu as tsa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex, keys0, pay0, roots = execution
    tree = mt.MemoryTree(H)
    assert tree.load(keys0, pay0) == (0, 0)
    status, info, image_pay, image_sib = tree.open(keys0)  # the freshly loaded tree: the image the execution starts from
    assert (status, info) == (0, 0) and (image_pay == pay0).all()
    segments, said = [], []
    for lo, hi in zip(CUTS, CUTS[1:]):
        c = closed_with((torch, prover), segment_of(ex, lo, hi), public_connector=True, poseidon2=True, memory_tree=tree)
        g = statement(prover, c, prover.prove_segment(c.seg, logup=True))
        names = [a["name"] for a in c.airs]
        ci, mi = names.index("connector"), names.index("memory_merkle")
        said.append(prover.segment_public_values(g["descs"], g["proof"], [None if v is None else len(v) for v in g["public"]], mi))
        segments.append(g)
        c.close()
    assert prover.verify_segment_chain(segments, sa.connector_links(ci) + mt.memory_links(mi), tsa.NQ, 0) == (0, 0)
    root_before, root_after = said[0][:8], said[-1][8:]
    # the outputs: what the executor left in address space 2
    final = dict(leaf_of(loc, word) for loc, (word, _) in ex.final.items() if loc[0] == 2)
    out_keys = np.array(sorted(final), np.uint64)
    assert len(out_keys) >= 1 and (out_keys >> np.uint64(29) == 1).all()
    status, info, pay, sib = tree.open(out_keys)
    assert (status, info) == (0, 0) and (pay == np.array([final[int(x)] for x in out_keys], np.uint32)).all()
    assert mt.verify_opening(H, root_after, out_keys, pay, sib) == (0, 0)
    assert (said[1][8:] != root_after).any() and mt.verify_opening(H, said[1][8:], out_keys, pay, sib)[0] == 20  # segment 2's root_after: not this memory
    assert mt.verify_opening(H, root_before, out_keys, pay, sib)[0] == 20
    # the image: spot-checked, and whole
    assert mt.verify_opening(H, root_before, keys0, image_pay, image_sib) == (0, 0)
    assert mt.verify_opening(H, root_after, keys0, image_pay, image_sib)[0] == 20
    tree.close()
