"""The sparse memory Merkle tree on the device (powdr_amd/memory_tree.py, pw_memory_tree_*) against the numpy reference
of tests/_memory_tree_ref.py: roots, record rows, node ids, row counts and statuses, the records as the first sender on the compression
bus next to the Poseidon2 chip, and the three chained segments of tests/test_public_values_gpu.py with their memory roots. Every
comparison is exact. The sizes are the smallest at which each path is taken: TAIL_NODES is the library's kMemoryTreeTailNodes — a level
(or a touched node set) with more nodes than that goes through the per-level kernels, anything smaller is finished by one workgroup."""
import copy
import ctypes as C
import itertools

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _chained_vm as vm
from tests import _memory_tree_ref as ref
from tests.test_bus_check_gpu import from_dev

pytestmark = pytest.mark.gpu
P = om.P
NQ = 4
BUS = 5
H = 30
TAIL_NODES = 1024  # powdr_amd/csrc/memory_tree.hip kMemoryTreeTailNodes
CUTS = (0, 5, 9, 12)  # tests/test_public_values_gpu.py


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


def payloads(rng, n):
    return rng.integers(0, P, (n, 8), dtype=np.uint32)


def checked_update(tree, want, keys, init, fin, **kw):
    """one update on the device tree and on the reference `want`: records, node ids, n_rows, log_height and root equal"""
    status, info, (trace, ids), lh, rows = tree.update(keys, init, fin, node_ids=True, **kw)
    m, want_ids, want_lh, want_rows = want.update(keys, init, fin)
    assert (status, info, lh, rows) == (0, 0, want_lh, want_rows)
    got = from_dev(trace).reshape(25, 1 << lh)
    assert (got == m).all(), np.argwhere(got != m)[:5]
    assert (ids.cpu().numpy().view(np.uint64) == want_ids).all()
    assert (tree.root() == want.root()).all()
    return trace, ids


# ---- every leaf set at height 3 ---------------------------------------------------------------------------------------------------------
def test_every_leaf_set_at_height_3(gpu):
    from powdr_amd import memory_tree as mt

    k = constants()
    pay = payloads(np.random.default_rng(1), 8)
    for r in range(9):
        for keys in itertools.combinations(range(8), r):
            t, want = mt.MemoryTree(3), ref.SparseTree(3, k)
            assert t.load(list(keys), pay[list(keys)]) == (0, 0)
            want.write(keys, pay[list(keys)])
            assert (t.root() == want.root()).all(), keys
            assert t.stats()["leaves"] == r
            t.close()


# ---- edge keys at height 30 -------------------------------------------------------------------------------------------------------------
def random_keys(seed, n, space=1 << H):
    """n distinct keys scattered over the whole space, sorted"""
    rng = np.random.default_rng(seed)
    return np.sort(rng.choice(np.unique(rng.integers(0, space, 2 * n, dtype=np.uint64)), n, replace=False))


def clustered_and_scattered():
    base = np.uint64(0x12345000)
    return np.unique(np.concatenate([base + np.arange(2048, dtype=np.uint64), random_keys(7, 2048)]))


EDGE_KEYS = {
    "first": [0], "last": [(1 << H) - 1], "siblings": [0, 1], "neighbours": [1, 2], "meet_at_the_root": [(1 << 29) - 1, 1 << 29],
    "random_3": random_keys(3, 3), "consecutive_255": 1000 + np.arange(255), "consecutive_256": 1000 + np.arange(256),
    "consecutive_257": 1000 + np.arange(257), "random_1000": random_keys(4, 1000),
    # the tail threshold: a level 0 of TAIL_NODES nodes is finished by the tail, one more takes a level kernel; 2 * TAIL_NODES + 1
    # consecutive keys leave TAIL_NODES + 1 nodes on level 1 too; scattered keys stay above the threshold for twenty levels
    "consecutive_tail": 77 + np.arange(TAIL_NODES), "consecutive_tail_plus_1": 77 + np.arange(TAIL_NODES + 1),
    "consecutive_two_tails_plus_1": 77 + np.arange(2 * TAIL_NODES + 1), "random_tail_plus_1": random_keys(5, TAIL_NODES + 1),
    "clustered_and_scattered_4096": clustered_and_scattered(),
}


@pytest.mark.parametrize("name", list(EDGE_KEYS))
def test_edge_keys_at_height_30(gpu, name):
    from powdr_amd import memory_tree as mt

    keys = np.asarray(EDGE_KEYS[name], dtype=np.uint64)
    n = len(keys)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and (name != "clustered_and_scattered_4096" or 4000 < n <= 4096)
    fin = payloads(np.random.default_rng(n), n)
    k = constants()
    # as an update of the empty tree (records), and as a load into a second tree: the same root
    t, want = mt.MemoryTree(H), ref.SparseTree(H, k)
    checked_update(t, want, keys, np.zeros((n, 8), np.uint32), fin)
    st = t.stats()
    assert st["leaves"] == n and st["stored_nodes"] == sum(len(lv) for lv in want.levels) and st["last_permutations"] == st["stored_nodes"]
    # at or below the threshold no level has a launch of its own: validate, lookup, scan, the touched sets (one workgroup), the leaves, the
    # tree (one workgroup), and the rows of level 0, the touched sets again, the rows of every level above
    assert st["device_bytes"] > 0 and (st["last_launches"] == 9 if n <= TAIL_NODES else 9 < st["last_launches"] < 400)
    loaded = mt.MemoryTree(H)
    assert loaded.load(keys, fin) == (0, 0) and (loaded.root() == want.root()).all()
    t.close()
    loaded.close()


# ---- a sequence of updates ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sequence():
    """2^12 loaded leaves; update A: 100 changed, 100 with init == fin, 100 new keys of which five end with the zero payload; update B on
    top: TAIL_NODES + 76 keys, stored and new -> the steps and the reference's answers"""
    k = constants()
    rng = np.random.default_rng(12)
    keys0 = random_keys(8, 1 << 12)
    pay0 = payloads(rng, 1 << 12)
    want = ref.SparseTree(H, k)
    want.write(keys0, pay0)
    root0 = want.root().copy()
    pick = np.sort(rng.choice(1 << 12, 200, replace=False))
    changed = set(rng.choice(pick, 100, replace=False).tolist())
    fresh = np.setdiff1d(random_keys(9, 140), keys0)[:100]
    keys_a = np.concatenate([keys0[pick], fresh])
    init_a = np.concatenate([pay0[pick], np.zeros((100, 8), np.uint32)])
    fin_a = init_a.copy()
    for j, i in enumerate(pick):
        if int(i) in changed:
            fin_a[j] = payloads(rng, 1)[0]
    fin_a[200:] = payloads(rng, 100)
    fin_a[200:205] = 0
    order = np.argsort(keys_a)
    keys_a, init_a, fin_a = keys_a[order], init_a[order], fin_a[order]
    a = want.update(keys_a, init_a, fin_a)
    root_a = want.root().copy()
    stored = np.array(sorted(want.payload), np.uint64)
    keys_b = np.unique(np.concatenate([rng.choice(stored, TAIL_NODES - 100, replace=False), np.setdiff1d(random_keys(10, 200), stored)[:176]]))
    assert len(keys_b) == TAIL_NODES + 76
    init_b = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys_b], np.uint32)
    fin_b = payloads(rng, len(keys_b))
    b = want.update(keys_b, init_b, fin_b)
    return dict(load=(keys0, pay0, root0), a=(keys_a, init_a, fin_a, a, root_a), b=(keys_b, init_b, fin_b, b, want.root().copy()),
                stored=sum(len(lv) for lv in want.levels))


def test_a_sequence_of_updates_equals_the_reference_and_repeats_byte_for_byte(gpu, sequence):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    runs = []
    for _ in range(2):
        t = mt.MemoryTree(H)
        keys0, pay0, root0 = sequence["load"]
        assert t.load(keys0, pay0) == (0, 0) and (t.root() == root0).all()
        out = []
        for step in ("a", "b"):
            keys, init, fin, (m, ids, lh, rows), root = sequence[step]
            status, info, (trace, got_ids), got_lh, got_rows = t.update(keys, init, fin, node_ids=True)
            assert (status, info, got_lh, got_rows) == (0, 0, lh, rows)
            got = from_dev(trace).reshape(25, 1 << lh)
            assert (got == m).all(), np.argwhere(got != m)[:5]
            assert (got_ids.cpu().numpy().view(np.uint64) == ids).all() and (t.root() == root).all()
            out += [trace.clone(), got_ids.clone()]
        assert t.stats()["stored_nodes"] == sequence["stored"]
        runs.append(out)
        t.close()
    assert all(torch.equal(x, y) for x, y in zip(*runs))


# ---- statuses ---------------------------------------------------------------------------------------------------------------------------
def test_statuses_leave_the_tree_as_it_was(gpu):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    k = constants()
    rng = np.random.default_rng(13)
    keys0 = random_keys(11, 300)
    pay0 = payloads(rng, 300)
    t, want = mt.MemoryTree(H), ref.SparseTree(H, k)
    assert t.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)

    def unchanged_and_still_usable():
        """the root is what it was, and a correct update (two stored leaves and a new one) then succeeds"""
        assert (t.root() == want.root()).all()
        new = int(rng.integers(0, 1 << H))
        while new in want.payload:
            new += 1
        keys = np.array(sorted([int(keys0[3]), int(keys0[200]), new]), np.uint64)
        init = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)
        checked_update(t, want, keys, init, payloads(rng, 3))

    keys = keys0[[5, 50, 120, 250]]
    init = np.array([want.payload[int(x)] for x in keys], np.uint32)
    fin = payloads(rng, 4)
    # 3: two leaves do not hold their init words: the smaller key is named
    bad = init.copy()
    bad[1, 7] = (int(bad[1, 7]) + 1) % P
    bad[3, 0] = (int(bad[3, 0]) + 1) % P
    assert t.update(keys, bad, fin) == (3, int(keys[1]), None, 1, 0)
    unchanged_and_still_usable()
    absent = np.array([int(keys0[-1]) + 1], np.uint64)  # a leaf that is not stored holds the zero payload
    assert int(absent[0]) not in want.payload and t.update(absent, payloads(rng, 1), payloads(rng, 1))[:2] == (3, int(absent[0]))
    unchanged_and_still_usable()
    # 4: a duplicate, a descending pair, a key >= 2^H: the index of the first offending key
    for wrong, at in ((keys[[0, 1, 1, 3]], 2), (keys[[0, 2, 1, 3]], 2), (np.array([int(keys[0]), int(keys[1]), 1 << H, (1 << H) + 1], np.uint64), 2)):
        assert t.update(wrong, init, fin)[:3] == (4, at, None)
        assert t.load(wrong, fin) == (4, at)
        unchanged_and_still_usable()
    # 5: a payload word that is no field element (Montgomery words on the device: the canonical door refuses it)
    to_dev = lambda a: torch.from_numpy(om.to_monty(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()
    for which in (0, 1):
        words = [to_dev(init), to_dev(fin)]
        words[which][8 * 2 + 5] = P
        assert t.update(keys, words[0], words[1])[:3] == (5, 2, None)
        unchanged_and_still_usable()
    # 1: a record buffer of 2^3 rows: the height comes back, the buffer is untouched
    _, _, want_lh, want_rows = copy.deepcopy(want).update(keys, init, fin)
    out = torch.full((25 << 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert t.update(keys, init, fin, cap_log_height=3, out=out) == (1, 0, None, want_lh, want_rows)
    assert bool((out == 0x5A5A5A5A).all()) and want_lh > 3
    unchanged_and_still_usable()
    # load mode with a record buffer, and NULL where a pointer is required: -1
    kd, fd = mt._keys(keys), to_dev(fin)
    lh, rows, status, info = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    u = mt.lib.pw_memory_tree_update
    assert u(t._h, kd.data_ptr(), None, fd.data_ptr(), 4, out.data_ptr(), None, 3, C.byref(lh), C.byref(rows), C.byref(status), C.byref(info)) == -1
    assert u(t._h, kd.data_ptr(), fd.data_ptr(), None, 4, None, None, 0, C.byref(lh), C.byref(rows), C.byref(status), C.byref(info)) == -1
    assert u(t._h, kd.data_ptr(), fd.data_ptr(), fd.data_ptr(), 4, None, None, 0, None, C.byref(rows), C.byref(status), C.byref(info)) == -1
    assert u(None, kd.data_ptr(), None, fd.data_ptr(), 4, None, None, 0, None, None, C.byref(status), C.byref(info)) == -1
    unchanged_and_still_usable()
    # without a buffer of the caller's the wrapper retries status 1 at the height asked for; without records nothing is written at all
    status, info, trace, lh_, rows_ = t.update(keys, init, fin, cap_log_height=3)
    m, _, _, _ = want.update(keys, init, fin)
    assert (status, lh_, rows_) == (0, want_lh, want_rows) and (from_dev(trace).reshape(25, -1) == m).all() and (t.root() == want.root()).all()
    assert t.update(keys, fin, init, records=False) == (0, 0, None, want_lh, want_rows)
    want.write(keys, init)
    assert (t.root() == want.root()).all()
    t.close()


# ---- the records on the compression bus ---------------------------------------------------------------------------------------------------
def test_the_records_and_the_chip_close_bus_5_and_prove(gpu, monkeypatch):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa

    monkeypatch.delenv("POWDR_LOGUP_INTERPRET", raising=False)
    k = constants()
    rng = np.random.default_rng(14)
    t, want = mt.MemoryTree(H), ref.SparseTree(H, k)
    keys0 = random_keys(15, 5)
    pay0 = payloads(rng, 5)
    assert t.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)
    keys = np.unique(np.concatenate([keys0[:3], random_keys(16, 2)]))  # three stored leaves, two new ones
    init = np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)
    trace, _ = checked_update(t, want, keys, init, payloads(rng, 5))
    lh = (trace.numel() // 25).bit_length() - 1
    rows = 2 * (5 + sum(len({int(x) >> l for x in keys}) for l in range(1, H + 1)))
    assert 200 < rows <= 1 << lh
    air, chip_air = mt.records_air(), sa.poseidon2_air()
    assert air.width == 25 and len(air.cons[1]) == 1 and np.asarray(air.inter[0]).tolist() == [[BUS, 24, 0]]
    rec = air.make_prover(NQ)
    assert rec.max_constraint_degree() == 2 and rec.check_constraints(trace.data_ptr(), lh) == (0, None, None)
    senders = [(rec, trace.data_ptr(), lh)]
    chip_trace, chip_lh, chip_rows, status = sa.poseidon2_compress_trace(senders, 4)
    assert status == 0 and chip_rows <= rows  # (a subtree that did not change is opened with the same tuple before and after)
    chip = chip_air.make_prover(NQ)
    seg = senders + [(chip, chip_trace.data_ptr(), chip_lh)]
    summaries, tuples = prover.check_segment_buses(seg, buses=[BUS])
    assert [(s["bus"], s["status"], s["n_unbalanced"]) for s in summaries] == [(BUS, 0, 0)] and tuples == [] and summaries[0]["n_active"] == rows + chip_rows
    descs = [air.description(lh), chip_air.description(chip_lh)]
    proofs = {}
    for jit in ("0", "1"):
        monkeypatch.setenv("POWDR_JIT", jit)
        ps = [air.make_prover(NQ), chip_air.make_prover(NQ)]
        proofs[jit] = prover.prove_segment([(ps[0], trace.data_ptr(), lh), (ps[1], chip_trace.data_ptr(), chip_lh)], logup=True)
        assert ps[1].specialised()["state"] == (1 if jit == "1" else 0)
        rc, total = prover.verify_segment(descs, proofs[jit], NQ, 0, True, check_balance=True)
        assert rc == 0 and not np.asarray(total).any()
        for p in ps:
            p.close()
    monkeypatch.delenv("POWDR_JIT")
    assert len(proofs["0"]) == len(proofs["1"]) and (proofs["0"] == proofs["1"]).all()
    # one `out` word of one record changed (the new root): the bus check names that tuple and the chip's
    ROW = rows - 1
    honest = from_dev(trace).reshape(25, -1)[1:, ROW].tolist()
    bad = trace.clone()
    bad[(17 + 5) * (1 << lh) + ROW] = int(om.to_monty(np.array([(honest[16 + 5] + 1) % P], np.uint32))[0])
    summaries, tuples = prover.check_segment_buses([(rec, bad.data_ptr(), lh), seg[1]], buses=[BUS])
    assert summaries == [dict(bus=BUS, status=1, n_active=rows + chip_rows, n_unbalanced=2)] and len(tuples) == 2
    sent = next(x for x in tuples if x["net_multiplicity"] == 1)
    lost = next(x for x in tuples if x["net_multiplicity"] == P - 1)
    assert (sent["air"], sent["interaction"], sent["row"], sent["n_args"]) == (0, 0, ROW, 24)
    assert sent["args"] == honest[:len(sent["args"])] == lost["args"] and lost["air"] == 1
    assert from_dev(chip_trace).reshape(307, -1)[1:17, lost["row"]].tolist() == honest[:16]
    rec.close()
    chip.close()
    t.close()


# ---- three chained segments ---------------------------------------------------------------------------------------------------------------
def leaf_of(location, word):
    space, ptr = location
    return ((space - 1) << 29) + ptr, [(word >> (8 * i)) & 0xFF for i in range(4)] + [0] * 4


@pytest.fixture(scope="module")
def chain(gpu):
    """one execution of 12 calls cut into segments of 5, 4 and 3 calls, each closed (close_segment as it is) -> (execution, per segment
    the boundary AIR's (trace, log_h, locations))"""
    from tests import test_system_airs_gpu as tsa

    ex = vm.Execution(CUTS[-1], seed=5)
    segments = []
    for lo, hi in zip(CUTS, CUTS[1:]):
        piece = copy.copy(ex)
        piece.rec, piece.calls = np.ascontiguousarray(ex.rec[:, lo:hi]), hi - lo
        c = tsa.Closed(gpu, piece)
        b = c.by_name("boundary")
        segments.append((b["trace"].clone(), b["log_h"], int(from_dev(b["trace"]).reshape(18, -1)[0].sum())))
        c.close()
    return ex, segments


def test_boundary_leaves_equal_a_numpy_reading_of_the_trace(gpu, chain):
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa

    col = {n: i for i, n in enumerate(sa.BOUNDARY_COLUMNS)}
    for trace, lh, n in chain[1]:
        m = from_dev(trace).reshape(18, 1 << lh).astype(np.uint64)
        assert n >= 2 and m[col["is_valid"], :n].all() and not m[col["is_valid"], n:].any()
        keys, init, fin = mt.boundary_leaves(trace, lh, n)
        want_keys = (m[col["as"], :n] - 1) * (1 << 29) + m[col["ptr"], :n]
        assert (keys.cpu().numpy().view(np.uint64) == want_keys).all() and (np.diff(want_keys.astype(np.int64)) > 0).all()
        for got, first in ((init, col["init0"]), (fin, col["fin0"])):
            g = from_dev(got).reshape(n, 8)
            assert (g[:, :4] == m[first:first + 4, :n].T).all() and not g[:, 4:].any()


def test_the_roots_of_three_chained_segments_and_a_skipped_segment(gpu, chain):
    from powdr_amd import memory_tree as mt

    ex, segments = chain
    k = constants()
    leaves = dict(leaf_of(loc, word) for loc, (word, _) in ex.initial.items())
    keys0 = np.array(sorted(leaves), np.uint64)
    pay0 = np.array([leaves[int(x)] for x in keys0], np.uint32)
    want = ref.SparseTree(H, k)
    want.write(keys0, pay0)
    roots = [want.root().copy()]
    for cut in CUTS[1:]:  # the executor's memory at every cut: the same execution stopped there
        part = vm.Execution(cut, seed=5)
        assert (part.rec == ex.rec[:, :cut]).all()
        now = dict(leaf_of(loc, word) for loc, (word, _) in part.final.items())
        want.write(sorted(now), np.array([now[x] for x in sorted(now)], np.uint32))
        roots.append(want.root().copy())
    assert len({r.tobytes() for r in roots}) == 4

    t = mt.MemoryTree(H)
    assert t.load(keys0, pay0) == (0, 0) and (t.root() == roots[0]).all()
    for (trace, lh, n), root in zip(segments, roots[1:]):
        keys, init, fin = mt.boundary_leaves(trace, lh, n)
        status, info, records, rec_lh, rows = t.update(keys, init, fin)
        assert (status, info) == (0, 0) and (t.root() == root).all()
        out = from_dev(records).reshape(25, -1)[17:]
        assert (out[:, rows - 1] == root).all() and rows >= 2 * n
    t.close()
    # segment 3 fed before segment 2: it does not start from the memory segment 1 left — a key that segment 2 wrote
    t = mt.MemoryTree(H)
    assert t.load(keys0, pay0) == (0, 0)
    assert t.update(*mt.boundary_leaves(*segments[0]), records=False)[:2] == (0, 0)
    k2, i2, f2 = mt.boundary_leaves(*segments[1])
    k3, i3, f3 = mt.boundary_leaves(*segments[2])
    written = set(k2.cpu().numpy().view(np.uint64)[(i2 != f2).any(dim=1).cpu().numpy()].tolist())
    status, info, records, _, _ = t.update(k3, i3, f3)
    assert status == 3 and records is None and info in written and (t.root() == roots[1]).all()
    assert t.update(k2, i2, f2, records=False)[:2] == (0, 0) and t.update(k3, i3, f3, records=False)[:2] == (0, 0)
    assert (t.root() == roots[3]).all()
    t.close()
