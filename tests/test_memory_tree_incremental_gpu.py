"""The incremental mode of the memory tree (pw_memory_tree_set_mode, MemoryTree(incremental=True)) against the numpy
reference of tests/_memory_tree_ref.py, which re-hashes only the touched paths too, and against a twin tree in rebuild mode: records,
node ids, row counts, roots and statuses exact, last_permutations against n + sum_(l=1..L) |T_l| + sum_(l>L) s_l computed from the
reference's level sizes and the keys, and every stored digest read back through an update that names every stored leaf.

The shapes are the smallest that reach each path. L = the number of levels l >= 1 whose level l - 1 holds more than TAIL_NODES nodes:
those are merged by touched_parent_kernel + move_kernel, everything above by the one-workgroup tail. 4096 scattered keys keep L = 20;
1000 keys keep the whole tree in the tail block (L = 0) and 100 more lift it out; 1025 and 2049 consecutive keys give L = 1 and 2. The
reference is computed once per module (the `image` fixture) and replayed."""
import copy

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _memory_tree_ref as ref
from tests.test_bus_check_gpu import from_dev
from tests.test_memory_tree_gpu import EDGE_KEYS, checked_update, payloads, random_keys

pytestmark = pytest.mark.gpu
P = om.P
H = 30
TAIL_NODES = 1024  # powdr_amd/csrc/memory_tree.hip kMemoryTreeTailNodes
BUS = 5
NQ = 4


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


def level_sizes(want):
    return [len(lv) for lv in want.levels]


def merged_levels(sizes):
    """L of a tree with these stored nodes per level"""
    return sum(1 for l in range(1, H + 1) if sizes[l - 1] > TAIL_NODES)


def incremental_permutations(keys, sizes):
    """n + sum_(l=1..L) |T_l| + sum_(l>L) s_l, from the keys and the NEW tree's stored nodes per level"""
    L = merged_levels(sizes)
    t = np.unique(np.asarray(keys, dtype=np.uint64))
    total = len(t)
    for l in range(1, H + 1):
        t = np.unique(t >> np.uint64(1))
        total += len(t) if l <= L else sizes[l]
    return total


def rebuild_permutations(keys, sizes):
    return len(keys) + sum(sizes[1:])


def held(want, keys):
    return np.array([want.payload.get(int(x), np.zeros(8, np.uint32)) for x in keys], np.uint32)


class Replay:
    """what checked_update asks of a reference, answered from a step computed before"""

    def __init__(self, step):
        self.step = step

    def update(self, keys, init, fin):
        return self.step["answer"]

    def root(self):
        return self.step["root"]


# ---- 1. a sequence of updates on an image of 4096 scattered leaves ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def image():
    """random_keys(8, 4096) loaded, then on one tree: one stored key; the new keys 0 and 2^30 - 1; a new key k ^ 1 whose parent exists;
    updates A and B as tests/test_memory_tree_gpu.py `sequence` makes them; every stored key rewritten; every stored key and as many new
    ones interleaved -> the steps with the reference's answers, and the reference as it was after the load"""
    k = constants()
    rng = np.random.default_rng(12)
    keys0 = random_keys(8, 1 << 12)
    pay0 = payloads(rng, 1 << 12)
    want = ref.SparseTree(H, k)
    want.write(keys0, pay0)
    loaded = copy.deepcopy(want)
    steps = []

    def step(name, keys, fin, init=None):
        keys = np.asarray(keys, dtype=np.uint64)
        assert (np.diff(keys.astype(np.int64)) > 0).all()
        init = held(want, keys) if init is None else init
        answer = want.update(keys, init, fin)
        steps.append(dict(name=name, keys=keys, init=init, fin=np.asarray(fin, np.uint32), answer=answer, root=want.root().copy(), sizes=level_sizes(want)))

    step("one_stored_key", keys0[[1234]], payloads(rng, 1))
    assert 0 not in want.payload and (1 << H) - 1 not in want.payload
    step("first_and_last_key", [0, (1 << H) - 1], payloads(rng, 2))
    lonely = next(int(x) for x in keys0[2000:] if int(x) ^ 1 not in want.payload)
    before = level_sizes(want)
    step("sibling_of_a_stored_key", [lonely ^ 1], payloads(rng, 1))
    assert [a - b for a, b in zip(steps[-1]["sizes"], before)] == [1] + [0] * H  # only level 0 grows: the parent exists
    # A: 200 stored keys of which 100 change, 100 new keys of which five end with the zero payload
    stored = np.array(sorted(want.payload), np.uint64)
    pick = np.sort(rng.choice(len(stored), 200, replace=False))
    changed = set(rng.choice(pick, 100, replace=False).tolist())
    fresh = np.setdiff1d(random_keys(9, 140), stored)[:100]
    keys_a = np.concatenate([stored[pick], fresh])
    fin_a = held(want, keys_a)
    for j, i in enumerate(pick):
        if int(i) in changed:
            fin_a[j] = payloads(rng, 1)[0]
    fin_a[200:] = payloads(rng, 100)
    fin_a[200:205] = 0
    order = np.argsort(keys_a)
    step("a", keys_a[order], fin_a[order])
    # B: TAIL_NODES + 76 keys, stored and new: the touched sets and the tree's levels both take the per-level path
    stored = np.array(sorted(want.payload), np.uint64)
    keys_b = np.unique(np.concatenate([rng.choice(stored, TAIL_NODES - 100, replace=False), np.setdiff1d(random_keys(10, 200), stored)[:176]]))
    assert len(keys_b) == TAIL_NODES + 76
    step("b", keys_b, payloads(rng, len(keys_b)))
    stored = np.array(sorted(want.payload), np.uint64)
    step("every_stored_key", stored, payloads(rng, len(stored)))
    more = np.setdiff1d(random_keys(11, len(stored) + 64), stored)[:len(stored)]
    both = np.unique(np.concatenate([stored, more]))
    assert len(both) == 2 * len(stored)
    step("larger_than_the_tree", both, payloads(rng, len(both)))
    final = np.array(sorted(want.payload), np.uint64)
    return dict(load=(keys0, pay0, loaded.root().copy()), loaded=loaded, load_sizes=level_sizes(loaded), steps=steps, final=(final, held(want, final)))


def run_steps(mt, torch, image, incremental, check):
    """the sequence on a fresh tree -> (tree, every trace and id array). check: each step against the reference's answer, and
    last_permutations against the formula of the tree's mode"""
    t = mt.MemoryTree(H, incremental=incremental)
    keys0, pay0, root0 = image["load"]
    assert t.load(keys0, pay0) == (0, 0) and (t.root() == root0).all()
    assert t.stats()["last_permutations"] == rebuild_permutations(keys0, image["load_sizes"])  # load mode: the full rebuild in both modes
    out = []
    for s in image["steps"]:
        if check:
            trace, ids = checked_update(t, Replay(s), s["keys"], s["init"], s["fin"])
        else:
            status, info, (trace, ids), lh, rows = t.update(s["keys"], s["init"], s["fin"], node_ids=True)
            assert (status, info, lh, rows) == (0, 0) + s["answer"][2:], s["name"]
        st = t.stats()
        want = (incremental_permutations if incremental else rebuild_permutations)(s["keys"], s["sizes"])
        print(s["name"], "keys", len(s["keys"]), "L", merged_levels(s["sizes"]), "permutations", st["last_permutations"], "want", want, "launches", st["last_launches"],
              "scratch", st["last_scratch_bytes"])
        assert st["last_permutations"] == want, s["name"]
        assert st["leaves"] == s["sizes"][0] and st["stored_nodes"] == sum(s["sizes"]), s["name"]
        out += [trace.clone(), ids.clone()]
    return t, out


def read_everything(t, image):
    """one update that names every stored key with init == fin == its payload: the rows open every stored node of the tree"""
    keys, pay = image["final"]
    status, info, (trace, ids), lh, rows = t.update(keys, pay, pay, node_ids=True)
    assert (status, info) == (0, 0)
    return [trace.clone(), ids.clone()]


def test_a_sequence_of_incremental_updates_equals_the_reference(gpu, image):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    assert merged_levels(image["load_sizes"]) == 20  # stored levels stay above TAIL_NODES through level 19
    assert [merged_levels(s["sizes"]) >= 20 for s in image["steps"]] == [True] * 7
    n_t0 = [len(s["keys"]) for s in image["steps"]]
    assert n_t0[:3] == [1, 2, 1] and n_t0[3] == 300 and n_t0[4] > TAIL_NODES and n_t0[5] == image["steps"][4]["sizes"][0] and n_t0[6] == 2 * n_t0[5]
    t, _ = run_steps(mt, torch, image, True, check=True)
    # the incremental updates hash less than a rebuild would whenever something stays untouched
    s = image["steps"][0]
    assert incremental_permutations(s["keys"], s["sizes"]) < rebuild_permutations(s["keys"], s["sizes"]) // 10
    t.close()


def test_every_stored_byte_equals_a_rebuild_mode_twin_and_a_second_run(gpu, image):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    runs = []
    for incremental in (True, False, True):
        t, out = run_steps(mt, torch, image, incremental, check=False)
        assert t.incremental is incremental
        out += read_everything(t, image)
        st = t.stats()
        runs.append((out, st["leaves"], st["stored_nodes"], t.root()))
        t.close()
    first, twin, second = runs
    for other in (twin, second):
        assert len(first[0]) == len(other[0]) == 16 and all(torch.equal(x, y) for x, y in zip(first[0], other[0]))
        assert first[1:3] == other[1:3] and (first[3] == other[3]).all()


# ---- 2. crossing the threshold ------------------------------------------------------------------------------------------------------------
def stats_after(t, twin, want, keys):
    """the incremental tree's count against the formula, the twin's against the rebuild's; both hold what the reference holds"""
    sizes = level_sizes(want)
    st, sw = t.stats(), twin.stats()
    print("keys", len(keys), "sizes", sizes[:4], "L", merged_levels(sizes), "permutations", st["last_permutations"], "rebuild", sw["last_permutations"])
    assert st["last_permutations"] == incremental_permutations(keys, sizes) and sw["last_permutations"] == rebuild_permutations(keys, sizes)
    assert st["leaves"] == sw["leaves"] == sizes[0] and st["stored_nodes"] == sw["stored_nodes"] == sum(sizes)
    return st, sw


def test_a_tree_in_the_tail_block_is_lifted_out_of_it(gpu):
    from powdr_amd import memory_tree as mt

    k = constants()
    rng = np.random.default_rng(21)
    keys0 = random_keys(4, 1000)
    pay0 = payloads(rng, 1000)
    t, twin, want = mt.MemoryTree(H, incremental=True), mt.MemoryTree(H), ref.SparseTree(H, k)
    assert t.load(keys0, pay0) == (0, 0) and twin.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)
    assert merged_levels(level_sizes(want)) == 0
    # L = 0: nothing is merged above level 0, the tail hashes every stored node above the leaves exactly as the rebuild does
    keys = np.sort(rng.choice(keys0, 10, replace=False))
    fin = payloads(rng, 10)
    checked_update(twin, copy.deepcopy(want), keys, held(want, keys), fin)
    checked_update(t, want, keys, held(want, keys), fin)
    st, sw = stats_after(t, twin, want, keys)
    assert st["last_permutations"] == sw["last_permutations"] == 10 + st["stored_nodes"] - st["leaves"]
    # 100 new scattered keys: the old levels live in the tail block, the new ones in buffers of their own
    keys = np.setdiff1d(random_keys(22, 140), keys0)[:100]
    fin = payloads(rng, 100)
    checked_update(twin, copy.deepcopy(want), keys, held(want, keys), fin)
    checked_update(t, want, keys, held(want, keys), fin)
    assert merged_levels(level_sizes(want)) >= 1 and level_sizes(want)[0] == 1100
    stats_after(t, twin, want, keys)
    # and one more small update, now from buffers of their own
    keys = np.sort(np.concatenate([rng.choice(keys0, 3, replace=False), keys[[7]], np.array([int(keys0[-1]) + 2], np.uint64)]))
    fin = payloads(rng, len(keys))
    checked_update(twin, copy.deepcopy(want), keys, held(want, keys), fin)
    checked_update(t, want, keys, held(want, keys), fin)
    st, sw = stats_after(t, twin, want, keys)
    assert st["last_permutations"] < sw["last_permutations"]
    t.close()
    twin.close()


@pytest.mark.parametrize("n_loaded, new, L, level_1", [(TAIL_NODES, [77 + TAIL_NODES], 1, 513), (2 * TAIL_NODES + 1, None, 2, 1025)])
def test_consecutive_keys_around_the_threshold(gpu, n_loaded, new, L, level_1):
    from powdr_amd import memory_tree as mt

    k = constants()
    rng = np.random.default_rng(n_loaded)
    keys0 = np.uint64(77) + np.arange(n_loaded, dtype=np.uint64)
    pay0 = payloads(rng, n_loaded)
    t, twin, want = mt.MemoryTree(H, incremental=True), mt.MemoryTree(H), ref.SparseTree(H, k)
    assert t.load(keys0, pay0) == (0, 0) and twin.load(keys0, pay0) == (0, 0)
    want.write(keys0, pay0)
    keys = np.array(new, np.uint64) if new else keys0[[0, 1024, 2048]]  # one key that lifts level 0 over the threshold / three stored keys
    fin = payloads(rng, len(keys))
    checked_update(twin, copy.deepcopy(want), keys, held(want, keys), fin)
    checked_update(t, want, keys, held(want, keys), fin)
    sizes = level_sizes(want)
    assert merged_levels(sizes) == L and sizes[1] == level_1 and sizes[2] == 513 - (L == 1) * 256
    stats_after(t, twin, want, keys)
    t.close()
    twin.close()


# ---- 3. the empty tree ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["siblings", "random_tail_plus_1", "clustered_and_scattered_4096"])
def test_an_incremental_update_of_the_empty_tree(gpu, name):
    from powdr_amd import memory_tree as mt

    keys = np.asarray(EDGE_KEYS[name], dtype=np.uint64)
    n = len(keys)
    fin = payloads(np.random.default_rng(n), n)
    t, want = mt.MemoryTree(H, incremental=True), ref.SparseTree(H, constants())
    checked_update(t, want, keys, np.zeros((n, 8), np.uint32), fin)
    sizes = level_sizes(want)
    st = t.stats()
    # every node is touched: the merge hashes what a rebuild hashes
    assert st["last_permutations"] == incremental_permutations(keys, sizes) == rebuild_permutations(keys, sizes) == st["stored_nodes"] == sum(sizes)
    assert st["leaves"] == n and (merged_levels(sizes) > 0) == (n > TAIL_NODES)
    t.close()


# ---- 5. statuses ------------------------------------------------------------------------------------------------------------------------------
def test_statuses_leave_an_incremental_tree_as_it_was_and_the_mode_changes_between_updates(gpu, image):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt

    rng = np.random.default_rng(23)
    keys0, pay0, root0 = image["load"]
    want = copy.deepcopy(image["loaded"])
    t = mt.MemoryTree(H, incremental=True)
    assert t.load(keys0, pay0) == (0, 0)
    keys = keys0[[5, 700, 2100, 4000]]
    init = held(want, keys)
    fin = payloads(rng, 4)
    to_dev = lambda a: torch.from_numpy(om.to_monty(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()
    before = t.stats()
    # 4: a descending pair; 5: a payload word that is no field element; 3: two leaves that do not hold their init words; 1: a short buffer
    assert t.update(keys[[0, 2, 1, 3]], init, fin)[:3] == (4, 2, None) and (t.root() == root0).all()
    words = to_dev(fin)
    words[8 * 2 + 5] = P
    assert t.update(keys, to_dev(init), words)[:3] == (5, 2, None) and (t.root() == root0).all()
    bad = init.copy()
    bad[1, 7] = (int(bad[1, 7]) + 1) % P
    bad[3, 0] = (int(bad[3, 0]) + 1) % P
    assert t.update(keys, bad, fin) == (3, int(keys[1]), None, 1, 0) and (t.root() == root0).all()
    _, _, want_lh, want_rows = copy.deepcopy(want).update(keys, init, fin)
    out = torch.full((25 << 3,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    assert t.update(keys, init, fin, cap_log_height=3, out=out) == (1, 0, None, want_lh, want_rows)
    assert bool((out == 0x5A5A5A5A).all()) and want_lh > 3 and (t.root() == root0).all()
    after = t.stats()
    assert {x: after[x] for x in ("leaves", "stored_nodes", "device_bytes")} == {x: before[x] for x in ("leaves", "stored_nodes", "device_bytes")}
    # a correct update then succeeds
    checked_update(t, want, keys, init, fin)
    assert t.stats()["last_permutations"] == incremental_permutations(keys, level_sizes(want))
    # rebuild -> incremental -> rebuild between three updates of one tree
    for incremental in (False, True, False):
        t.incremental = incremental
        new = int(rng.integers(0, 1 << H))
        while new in want.payload:
            new += 1
        keys = np.array(sorted([int(keys0[int(rng.integers(0, 4096))]), int(keys0[3000]), new]), np.uint64)
        checked_update(t, want, keys, held(want, keys), payloads(rng, 3))
        count = incremental_permutations if incremental else rebuild_permutations
        assert t.incremental is incremental and t.stats()["last_permutations"] == count(keys, level_sizes(want))
    t.close()


# ---- 6. the records of an incremental update on the compression bus ---------------------------------------------------------------------------
def test_the_records_of_an_incremental_update_and_the_chip_close_bus_5(gpu, image):
    torch, prover = gpu
    from powdr_amd import memory_tree as mt
    from powdr_amd import system_airs as sa

    rng = np.random.default_rng(24)
    keys0, pay0, _ = image["load"]
    t = mt.MemoryTree(H, incremental=True)
    assert t.load(keys0, pay0) == (0, 0)
    keys = np.unique(np.concatenate([keys0[[10, 11, 3000]], np.setdiff1d(random_keys(16, 4), keys0)[:2]]))  # three stored leaves, two new ones
    init = held(image["loaded"], keys)
    status, info, trace, lh, rows = t.update(keys, init, payloads(rng, 5))
    assert (status, info) == (0, 0) and rows == 2 * (5 + sum(len({int(x) >> l for x in keys}) for l in range(1, H + 1)))
    rec = mt.records_air().make_prover(NQ)
    senders = [(rec, trace.data_ptr(), lh)]
    chip_trace, chip_lh, chip_rows, status = sa.poseidon2_compress_trace(senders, 4)
    chip = sa.poseidon2_air().make_prover(NQ)
    summaries, tuples = prover.check_segment_buses(senders + [(chip, chip_trace.data_ptr(), chip_lh)], buses=[BUS])
    assert (status, summaries, tuples) == (0, [dict(bus=BUS, status=0, n_active=rows + chip_rows, n_unbalanced=0)], [])
    rec.close()
    chip.close()
    t.close()
