"""The memory Merkle AIR on the device (powdr_amd/memory_tree.py merkle_air / merkle_trace, pw_memory_merkle_trace,
system_airs.close_segment(memory_tree=)): the device trace against the numpy reference of tests/_memory_merkle_ref.py
word for word, the statuses, the three buses in the bus check, and the three chained segments of tests/test_memory_tree_gpu.py proven
with their memory roots as public values and linked by the chain verifier. Every comparison is exact. The sizes are the smallest at
which each path is taken: one workgroup is 256 rows, and the tree's own thresholds are those of tests/test_memory_tree_gpu.py."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _chained_vm as vm
from tests import _memory_merkle_ref as mref
from tests import _memory_tree_ref as tref
from tests.test_bus_check_gpu import from_dev, to_dev
from tests.test_memory_tree_gpu import CUTS, leaf_of, random_keys

pytestmark = pytest.mark.gpu
P = om.P
NQ = 4
H = 30
SENTINEL = 0x5A5A5A5A
NO_CONS = (np.zeros(0, np.uint32), np.zeros((0, 2), np.uint32))


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


def leaf_words(rng, n, bound=256):
    """n payloads as the memory has them: four words (bytes, as the boundary AIR sends them, or any field element), then four zeros —
    the Merkle AIR's leaf rows state those zeros"""
    w = np.zeros((n, 8), np.uint32)
    w[:, :4] = rng.integers(0, bound, (n, 4))
    return w


def init_of(want, keys):
    return np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)


def checked_trace(mt, tree, want, keys, init, fin, checker=None):
    """one update on the device tree and on the reference `want`, then the Merkle trace from the device's records against the reference's
    built from the reference's records: every word, the height, the node count; two runs give the same bytes; checker (a Prover of
    merkle_air): no constraint is violated with the roots as public values -> (trace, log_height, reference columns, where, public)"""
    import torch

    root_before = tree.root()
    status, info, (records, ids), lh, rows = tree.update(keys, init, fin, node_ids=True)
    m, want_ids, want_lh, want_rows = want.update(keys, init, fin)
    assert (status, info, lh, rows) == (0, 0, want_lh, want_rows)
    cols, where = mref.trace(m, want_ids, want_rows, tree.height)
    trace, mlh, nodes, status = mt.merkle_trace(records, ids, lh, rows, tree.height)
    assert (status, nodes, 1 << mlh) == (0, rows // 2, cols.shape[1])
    got = from_dev(trace).reshape(mref.WIDTH, 1 << mlh)
    assert (got == cols).all(), np.argwhere(got != cols)[:5]
    again = mt.merkle_trace(records, ids, lh, rows, tree.height)
    assert again[1:] == (mlh, nodes, 0) and torch.equal(again[0], trace)
    public = np.concatenate([root_before, tree.root()]).astype(np.uint32)
    assert (public == mref.public_of(cols)).all()
    if checker is not None:
        checker.set_public_values(public)
        assert checker.check_constraints(trace.data_ptr(), mlh) == (0, None, None)
    return trace, mlh, cols, where, public


# ---- the device trace against the reference -----------------------------------------------------------------------------------------------
def test_every_leaf_set_at_height_3(gpu):
    from powdr_amd import memory_tree as mt

    k = constants()
    rng = np.random.default_rng(1)
    stored = [1, 2, 6]
    pay = leaf_words(rng, 3)
    base = tref.SparseTree(3, k)
    base.write(stored, pay)
    checker = mt.merkle_air(3).make_prover(NQ)
    for r in range(1, 9):
        for keys in itertools.combinations(range(8), r):
            t, want = mt.MemoryTree(3), copy.deepcopy(base)
            assert t.load(stored, pay) == (0, 0)
            checked_trace(mt, t, want, list(keys), init_of(want, keys), leaf_words(rng, r), checker)
            t.close()
    checker.close()


@pytest.fixture(scope="module")
def loaded():
    """4096 scattered leaves at height 30 -> (keys, payloads, the reference tree)"""
    keys0 = random_keys(8, 1 << 12)
    pay0 = leaf_words(np.random.default_rng(31), 1 << 12, P)
    want = tref.SparseTree(H, constants())
    want.write(keys0, pay0)
    return keys0, pay0, want


def scattered_1025(loaded):
    """1025 scattered keys: 700 of the stored leaves and 325 new ones"""
    keys0 = loaded[0]
    rng = np.random.default_rng(32)
    keys = np.unique(np.concatenate([rng.choice(keys0, 700, replace=False), np.setdiff1d(random_keys(33, 400), keys0)[:325]]))
    assert len(keys) == 1025
    return keys


H30_CASES = ["edge_keys", "consecutive_257", "scattered_1025_rebuild", "scattered_1025_incremental", "every_stored_leaf_unchanged"]


@pytest.mark.parametrize("name", H30_CASES)
def test_height_30(gpu, loaded, name):
    from powdr_amd import memory_tree as mt

    rng = np.random.default_rng(H30_CASES.index(name))
    checker = mt.merkle_air(H).make_prover(NQ)
    t = mt.MemoryTree(H, incremental=name.endswith("incremental"))
    if name.startswith("scattered"):
        keys0, pay0, want = loaded[0], loaded[1], copy.deepcopy(loaded[2])
        assert t.load(keys0, pay0) == (0, 0)
        keys = scattered_1025(loaded)
        fin = leaf_words(rng, len(keys), P)
    elif name == "every_stored_leaf_unchanged":
        keys = random_keys(34, 300)
        want = tref.SparseTree(H, constants())
        want.write(keys, leaf_words(rng, 300, P))
        assert t.load(keys, init_of(want, keys)) == (0, 0)
        fin = init_of(want, keys)
    else:
        want = tref.SparseTree(H, constants())
        stored = [1, 77, (1 << 29) + 5, (1 << 30) - 1]
        want.write(stored, leaf_words(rng, 4, P))
        assert t.load(stored, init_of(want, stored)) == (0, 0)
        keys = np.array([0, 1, 1 << 29, (1 << 30) - 1] if name == "edge_keys" else 1000 + np.arange(257), np.uint64)  # 257: more than one workgroup
        fin = leaf_words(rng, len(keys), P)
    trace, lh, cols, where, public = checked_trace(mt, t, want, keys, init_of(want, keys), fin, checker)
    if name == "every_stored_leaf_unchanged":
        assert (public[:8] == public[8:]).all() and (cols[mref.LEFT0:mref.LEFT1] == cols[mref.LEFT1:]).all()
    if name == "edge_keys":
        assert cols[mref.INDEX].max() == (1 << 30) - 1 and set(cols[mref.LEVEL, :len(where)].tolist()) == set(range(H + 1))
    checker.close()
    t.close()


# ---- statuses -----------------------------------------------------------------------------------------------------------------------------
def test_statuses_against_a_sentinel_filled_buffer(gpu):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    rng = np.random.default_rng(41)
    t = mt.MemoryTree(H)
    keys = random_keys(42, 40)
    status, info, (records, ids), lh, rows = t.update(keys, np.zeros((40, 8), np.uint32), leaf_words(rng, 40, P), node_ids=True)
    assert status == 0 and rows % 2 == 0
    want_lh = (rows // 2 - 1).bit_length()
    fresh = lambda cap: torch.full((mref.WIDTH << cap,), SENTINEL, dtype=torch.int32, device="cuda")
    untouched = lambda out: bool((out == SENTINEL).all())
    # 1: the buffer is too small: untouched, and the height to come back with
    out = fresh(3)
    assert want_lh > 3 and mt.merkle_trace(records, ids, lh, rows, H, cap_log_height=3, out=out) == (None, want_lh, rows // 2, 1) and untouched(out)
    # without a buffer of the caller's the wrapper retries at that height
    trace, got_lh, nodes, status = mt.merkle_trace(records, ids, lh, rows, H, cap_log_height=3)
    assert (got_lh, nodes, status) == (want_lh, rows // 2, 0) and trace.numel() == mref.WIDTH << want_lh
    # 2: no rows
    out = fresh(want_lh)
    assert mt.merkle_trace(records, ids, lh, 0, H, cap_log_height=want_lh, out=out) == (None, 1, 0, 2) and untouched(out)
    # 3: the two halves of the ids swapped
    swapped = torch.cat([ids[rows // 2:], ids[:rows // 2]]).contiguous()
    assert mt.merkle_trace(records, swapped, lh, rows, H, cap_log_height=want_lh, out=fresh(want_lh))[1:] == (want_lh, rows // 2, 3)
    # ... and ids whose last node is not the root (H, 0): the records of a taller tree's path
    assert mt.merkle_trace(records, ids, lh, rows, H - 1, cap_log_height=want_lh, out=fresh(want_lh))[3] == 3
    # -1 before any GPU call: an odd n_rows, H = 31, H = 0, a NULL pointer
    out = fresh(want_lh)
    lh_, nodes_, status_ = C.c_uint32(77), C.c_uint64(77), C.c_uint32(77)
    f = mt.lib.pw_memory_merkle_trace
    tail = (want_lh, C.byref(lh_), C.byref(nodes_), C.byref(status_))
    assert f(records.data_ptr(), lh, ids.data_ptr(), rows - 1, H, out.data_ptr(), *tail) == -1
    assert f(records.data_ptr(), lh, ids.data_ptr(), rows, 31, out.data_ptr(), *tail) == -1
    assert f(records.data_ptr(), lh, ids.data_ptr(), rows, 0, out.data_ptr(), *tail) == -1
    assert f(None, lh, ids.data_ptr(), rows, H, out.data_ptr(), *tail) == -1 and f(records.data_ptr(), lh, None, rows, H, out.data_ptr(), *tail) == -1
    assert f(records.data_ptr(), lh, ids.data_ptr(), rows, H, None, *tail) == -1
    assert f(records.data_ptr(), lh, ids.data_ptr(), rows, H, out.data_ptr(), want_lh, None, C.byref(nodes_), C.byref(status_)) == -1
    assert untouched(out) and (lh_.value, nodes_.value, status_.value) == (77, 77, 77)
    t.close()


# ---- the three buses in the bus check -----------------------------------------------------------------------------------------------------
def test_the_bus_check_closes_buses_5_8_9_and_names_a_changed_digest(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    rng = np.random.default_rng(51)
    t, want = mt.MemoryTree(H), tref.SparseTree(H, constants())
    keys0 = random_keys(52, 6)
    pay0 = leaf_words(rng, 6)
    assert t.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)
    keys = np.unique(np.concatenate([keys0[:3], random_keys(53, 2)]))
    init, fin = init_of(want, keys), leaf_words(rng, len(keys))
    air = mt.merkle_air(H)
    merkle = air.make_prover(NQ)
    trace, lh, cols, where, public = checked_trace(mt, t, want, keys, init, fin, merkle)
    leaf_cols, leaf_inter = mref.leaf_sender(keys, init, fin)  # the boundary AIR's leaf sends, without a boundary AIR
    leaf_lh = leaf_cols.shape[1].bit_length() - 1
    leaves = prover.Prover(10, *NO_CONS, num_queries=NQ, interactions=leaf_inter)
    leaf_trace = to_dev(torch, leaf_cols)
    torch.cuda.synchronize()
    senders = [(leaves, leaf_trace.data_ptr(), leaf_lh), (merkle, trace.data_ptr(), lh)]
    chip_trace, chip_lh, chip_rows, status = sa.poseidon2_compress_trace(senders, 4)
    assert status == 0 and chip_rows <= 2 * len(where)
    chip = sa.poseidon2_air().make_prover(NQ)
    seg = senders + [(chip, chip_trace.data_ptr(), chip_lh)]
    summaries, tuples = prover.check_segment_buses(seg, buses=[5, 8, 9])
    assert [(s["bus"], s["status"], s["n_unbalanced"]) for s in summaries] == [(5, 0, 0), (8, 0, 0), (9, 0, 0)] and tuples == []
    n = len(where)
    assert [s["n_active"] for s in summaries] == [2 * n + chip_rows, (n - 1) + (n - 1), 2 * len(keys)]
    # one out1 word of a mid-level row changed on the device: its compression and its send to its parent are named
    node = next(x for x in sorted(where) if x[0] == H // 2)
    row = where[node]
    honest = cols[:, row].tolist()
    bad = trace.clone()
    bad[(mref.OUT1 + 5) * (1 << lh) + row] = int(om.to_monty(np.array([(honest[mref.OUT1 + 5] + 1) % P], np.uint32))[0])
    summaries, tuples = prover.check_segment_buses([seg[0], (merkle, bad.data_ptr(), lh), seg[2]], buses=[5, 8, 9])
    assert [(s["bus"], s["status"], s["n_unbalanced"]) for s in summaries] == [(5, 1, 2), (8, 1, 2), (9, 0, 0)] and len(tuples) == 4
    sent5 = next(x for x in tuples if x["bus"] == 5 and x["net_multiplicity"] == 1)
    lost5 = next(x for x in tuples if x["bus"] == 5 and x["net_multiplicity"] == P - 1)
    assert (sent5["air"], sent5["interaction"], sent5["row"], sent5["n_args"]) == (1, 1, row, 24) and lost5["air"] == 2
    assert sent5["args"] == honest[mref.LEFT1:mref.LEFT1 + 16] == lost5["args"]
    sent8 = next(x for x in tuples if x["bus"] == 8 and x["net_multiplicity"] == 1)
    lost8 = next(x for x in tuples if x["bus"] == 8 and x["net_multiplicity"] == P - 1)
    assert (sent8["air"], sent8["interaction"], sent8["row"], sent8["n_args"]) == (1, 2, row, 18) and sent8["args"][:2] == list(node) == lost8["args"][:2]
    parent = where[(node[0] + 1, node[1] >> 1)]
    assert (lost8["air"], lost8["interaction"], lost8["row"]) == (1, 3 + (node[1] & 1), parent) and lost8["args"][2:10] == honest[mref.OUT0:mref.OUT0 + 8]
    for p in (leaves, merkle, chip):
        p.close()
    t.close()


# ---- three chained segments -----------------------------------------------------------------------------------------------------------------
def segment_of(ex, lo, hi):
    piece = copy.copy(ex)
    piece.rec, piece.calls = np.ascontiguousarray(ex.rec[:, lo:hi]), hi - lo
    return piece


def closed_with(gpu, piece, **kw):
    """tests/test_system_airs_gpu.Closed with close_segment's keywords set"""
    from powdr_amd import system_airs as sa
    from tests import test_system_airs_gpu as tsa

    real, calls = sa.close_segment, []

    def close_segment(*a, **k):
        calls.append(k)
        return real(*a, **k, **kw)

    mp = pytest.MonkeyPatch()
    mp.setattr(sa, "close_segment", close_segment)
    try:
        c = tsa.Closed(gpu, piece)
    finally:
        mp.undo()
    assert len(calls) == 1, "Closed did not go through system_airs.close_segment: the keywords were not applied"
    return c


def statement(prover, c, proof):
    return dict(descs=[(a["width"], a["log_h"], a["cons"][0], a["cons"][1], a["inter"]) for a in c.airs], proof=proof, public=[a.get("public") for a in c.airs],
                preprocessed=[None if a["pre"] is None else (a["pre"][1], a["prover"].preprocessed_root()) for a in c.airs], logup=True, check_balance=True)


@pytest.fixture(scope="module")
def execution():
    """the 12-call execution, its initial image as leaves, and the executor's memory roots at the cuts (built as
    tests/test_memory_tree_gpu.py builds them)"""
    ex = vm.Execution(CUTS[-1], seed=5)
    leaves = dict(leaf_of(loc, word) for loc, (word, _) in ex.initial.items())
    keys0 = np.array(sorted(leaves), np.uint64)
    pay0 = np.array([leaves[int(x)] for x in keys0], np.uint32)
    want = tref.SparseTree(H, constants())
    want.write(keys0, pay0)
    roots = [want.root().copy()]
    for cut in CUTS[1:]:
        part = vm.Execution(cut, seed=5)
        assert (part.rec == ex.rec[:, :cut]).all()
        now = dict(leaf_of(loc, word) for loc, (word, _) in part.final.items())
        want.write(sorted(now), np.array([now[x] for x in sorted(now)], np.uint32))
        roots.append(want.root().copy())
    assert len({r.tobytes() for r in roots}) == 4
    return ex, keys0, pay0, roots


def test_three_chained_segments_with_their_memory_roots(gpu, execution, monkeypatch):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa
    from tests import test_system_airs_gpu as tsa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    ex, keys0, pay0, roots = execution
    tree = mt.MemoryTree(H)
    assert tree.load(keys0, pay0) == (0, 0) and (tree.root() == roots[0]).all()
    closed, segments = [], []
    for s, (lo, hi) in enumerate(zip(CUTS, CUTS[1:])):
        c = closed_with((torch, prover), segment_of(ex, lo, hi), public_connector=True, poseidon2=True, memory_tree=tree)
        closed.append(c)
        names = [a["name"] for a in c.airs]
        assert names[names.index("boundary"):names.index("boundary") + 3] == ["boundary", "memory_merkle", "poseidon2"]
        # every bus balances, all nine
        summaries, tuples = prover.check_segment_buses(c.seg)
        assert [(x["bus"], x["status"]) for x in summaries] == [(b, 0) for b in (0, 1, 2, 3, 5, 6, 7, 8, 9)] and tuples == []
        for a in c.airs:
            assert a["prover"].check_constraints(a["trace"].data_ptr(), a["log_h"]) == (0, None, None), a["name"]
        # the Merkle AIR's public values are the executor's memory roots at the cuts
        mk = c.by_name("memory_merkle")
        assert (mk["public"] == np.concatenate([roots[s], roots[s + 1]])).all() and (tree.root() == roots[s + 1]).all()
        proofs = {}
        for jit in ("0", "1"):  # the same provers: never specialised while POWDR_JIT=0, specialised at the first proof with POWDR_JIT=1
            monkeypatch.setenv("POWDR_JIT", jit)
            proofs[jit] = prover.prove_segment(c.seg, logup=True)
            assert mk["prover"].specialised()["state"] == (1 if jit == "1" else 0)
        monkeypatch.delenv("POWDR_JIT")
        assert len(proofs["0"]) == len(proofs["1"]) and (proofs["0"] == proofs["1"]).all()
        g = statement(prover, c, proofs["0"])
        rc, total = prover.verify_segment(g["descs"], g["proof"], tsa.NQ, 0, True, check_balance=True, preprocessed=g["preprocessed"], public=g["public"])
        assert rc == 0 and not np.asarray(total).any()
        mi = names.index("memory_merkle")
        said = prover.segment_public_values(g["descs"], g["proof"], [None if v is None else len(v) for v in g["public"]], mi)
        assert (said == mk["public"]).all()
        segments.append(g)
    ci, mi = names.index("connector"), names.index("memory_merkle")
    assert all([a["name"] for a in c.airs].index("memory_merkle") == mi for c in closed)
    links = sa.connector_links(ci) + mt.memory_links(mi)
    assert len(links) == 10 and prover.verify_segment_chain(segments, links, tsa.NQ, 0) == (0, 0)
    # segments 2 and 3 swapped: segment 1 does not end where segment 3 starts — a timestamp or a memory link from segment 0
    rc, at = prover.verify_segment_chain([segments[0], segments[2], segments[1]], links, tsa.NQ, 0)
    assert rc == 18 and 1 <= at < len(links)
    # with the memory links alone: the memory of segment 1's end is not the memory segment 3 starts from
    rc, at = prover.verify_segment_chain([segments[0], segments[2], segments[1]], mt.memory_links(mi), tsa.NQ, 0)
    assert rc == 18 and at < 8
    # expected roots off by one word: the verifier compares what the proof carries with what it is told
    g = segments[1]
    wrong = list(g["public"])
    wrong[mi] = g["public"][mi].copy()
    wrong[mi][8 + 3] = (int(wrong[mi][8 + 3]) + 1) % P
    assert prover.verify_segment(g["descs"], g["proof"], tsa.NQ, 0, True, check_balance=True, preprocessed=g["preprocessed"], public=wrong)[0] == 17
    assert prover.verify_segment_chain([segments[0], dict(g, public=wrong), segments[2]], links, tsa.NQ, 0) == (17, 1)
    for c in closed:
        c.close()
    tree.close()
    # a fourth tree that skipped segment 2: segment 3 does not start from the memory segment 1 left
    tree = mt.MemoryTree(H)
    assert tree.load(keys0, pay0) == (0, 0)
    closed_with((torch, prover), segment_of(ex, CUTS[0], CUTS[1]), public_connector=True, poseidon2=True, memory_tree=tree).close()
    assert (tree.root() == roots[1]).all()
    with pytest.raises(ValueError, match=r"memory tree: status 3.*\(key \d+\)"):
        closed_with((torch, prover), segment_of(ex, CUTS[2], CUTS[3]), public_connector=True, poseidon2=True, memory_tree=tree)
    assert (tree.root() == roots[1]).all()  # the tree is what it was
    tree.close()


def test_the_default_is_unchanged(gpu, execution):
    """close_segment with memory_tree=None against a call made with the keyword absent: the same AIR names, the same proof words"""
    torch, prover = gpu
    ex = execution[0]
    got = []
    for kw in ({}, dict(memory_tree=None)):
        c = closed_with((torch, prover), segment_of(ex, CUTS[0], CUTS[1]), public_connector=True, **kw)
        got.append(([a["name"] for a in c.airs], prover.prove_segment(c.seg, logup=True)))
        assert "memory_merkle" not in got[-1][0] and np.asarray(c.by_name("boundary")["inter"][0]).shape[0] == 8
        c.close()
    assert got[0][0] == got[1][0] and len(got[0][1]) == len(got[1][1]) and (got[0][1] == got[1][1]).all()
