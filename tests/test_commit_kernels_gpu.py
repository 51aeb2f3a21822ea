"""The commitment kernels (csrc/merkle.hip) form by form, through their stage entry points, against tests/_commit_ref.py (the numpy
reference that tests/test_commit_ref_cpu.py ties to the oracle): leaf_hash_kernel with digest strides, leaf_absorb_kernel at every
(rate position carried in, width of the run) and along chains of matrix / pointer-table / streamed runs, leaf_hash_levels_kernel and
compress_strided_kernel over whole mixed trees (resident and external levels), the binary tree around its tail boundary, the FRI
leaves, and edge-valued words through the parked sponge states under the edge tables. Tests a-d and f run with POWDR_HASH_WAVES unset
(the <6> instantiations) and "8" (the <8> ones, built under a 64-VGPR cap). Every output buffer starts as a sentinel no kernel can
store, and the words a call must not write must still hold it. The arithmetic is exact: every comparison is equality of all words."""
import functools

import numpy as np
import pytest

from oracle import apc_model as om
from tests import _commit_ref as ref
from tests import _poseidon2_tables as tables
from tests.test_poseidon2_edge_tables import GPU_TABLES, installed

P = om.P
SENT = 0xFFFFFFFF  # digests are stored reduced (< p), parked states below 2p = 0xF0000002: no kernel stores this word


@pytest.fixture(scope="module")
def gpu():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs a GPU (run with -m gpu on the GPU box)")
    from powdr_amd import abi, prover

    return torch, abi, prover


@pytest.fixture(params=[None, "8"], ids=["waves_default", "waves_8"])
def waves(request, monkeypatch):
    """POWDR_HASH_WAVES, which the library reads per call: unset = the <6> leaf kernels, 8 = the <8> ones"""
    if request.param is None:
        monkeypatch.delenv("POWDR_HASH_WAVES", raising=False)
    else:
        monkeypatch.setenv("POWDR_HASH_WAVES", request.param)
    return request.param


def constants():
    from powdr_amd import prover

    return prover.poseidon2_constants()


def to_dev(torch, canonical):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(canonical, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()


def sentinel(torch, n_words):
    return torch.full((n_words,), -1, dtype=torch.int32, device="cuda")


def raw(t):
    return t.cpu().numpy().view(np.uint32)


def canonical(raw_words):
    return om.from_monty(np.ascontiguousarray(raw_words, dtype=np.uint32))


def matrix_form(torch, rng, rows, col_stride):
    """rows [h, w] canonical -> a device matrix with column c at c * col_stride; the padding behind a column holds other field words"""
    h, w = rows.shape
    assert col_stride >= h
    buf = rng.integers(0, P, (w, col_stride), dtype=np.uint32)
    buf[:, :h] = rows.T
    return to_dev(torch, buf)


def table_form(torch, rng, rows):
    """rows [h, w] canonical -> (the device buffer, a device array of w device column pointers): the columns sit in shuffled slots of h
    + 5 words, so neighbouring pointers are not neighbouring memory and a column is only 4-byte aligned"""
    h, w = rows.shape
    slot = h + 5
    order = rng.permutation(w)
    buf = rng.integers(0, P, (w, slot), dtype=np.uint32)
    buf[order, :h] = rows.T  # column c lives in slot order[c]
    d = to_dev(torch, buf)
    ptrs = torch.tensor([d.data_ptr() + int(order[c]) * slot * 4 for c in range(w)], dtype=torch.int64, device="cuda")
    return d, ptrs


# ---- a. leaf hash with strides ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("height", [1, 255, 257, 513])
def test_leaf_hash_with_digest_strides(gpu, waves, height):
    """pw_merkle_leaf_hash (leaf_hash_kernel): heights that are no power of two, widths around the rate, a column stride past the
    height; (digest_stride, offset) = (1, 0), then 2^b with every offset in shuffled order, each call on the matrix of the rows
    r + 2^b i: after one offset only its slots have changed, after all of them the leaves are the reference's over the whole matrix,
    and the slots behind the last row still hold the sentinel"""
    torch, abi, prover = gpu
    k = constants()
    rng = np.random.default_rng(height)
    tail = 4  # digest slots behind the last row
    for width in (1, 7, 8, 9, 17):
        rows = rng.integers(0, P, (height, width), dtype=np.uint32)
        want = ref.sponge(rows, k)
        for pad in (0, 3):
            d_m = matrix_form(torch, rng, rows, height + pad)
            d_d = sentinel(torch, (height + tail) * 8)
            abi.check(prover.lib.pw_merkle_leaf_hash(d_m.data_ptr(), height, width, height + pad, d_d.data_ptr(), 1, 0), "pw_merkle_leaf_hash")
            torch.cuda.synchronize()
            got = raw(d_d).reshape(-1, 8)
            assert (got[height:] == SENT).all(), (width, pad)
            assert (canonical(got[:height]) == want).all(), (width, pad)
            for b in (1, 2, 3):
                stride = 1 << b
                d_d = sentinel(torch, (height + tail) * 8)
                before = raw(d_d).reshape(-1, 8)
                for r in rng.permutation(stride).tolist():
                    sub = rows[r::stride]
                    if not len(sub):  # a height of 0 is refused, and nothing is written
                        assert prover.lib.pw_merkle_leaf_hash(d_m.data_ptr(), 0, width, height + pad, d_d.data_ptr(), stride, r) == -1
                        continue
                    d_s = matrix_form(torch, rng, sub, len(sub) + pad)
                    abi.check(prover.lib.pw_merkle_leaf_hash(d_s.data_ptr(), len(sub), width, len(sub) + pad, d_d.data_ptr(), stride, r),
                              "pw_merkle_leaf_hash")
                    torch.cuda.synchronize()
                    after = raw(d_d).reshape(-1, 8)
                    own = np.zeros(height + tail, bool)
                    own[r:height:stride] = True
                    assert (after[~own] == before[~own]).all(), (width, pad, b, r)
                    assert (canonical(after[own]) == want[r::stride]).all(), (width, pad, b, r)
                    before = after
                assert (before[height:] == SENT).all() and (canonical(before[:height]) == want).all(), (width, pad, b)


# ---- the run-by-run form ----------------------------------------------------------------------------------------------------------
def absorb(gpu, m_ptr, col_stride, cols_ptr, n_cols, pos0, height, row_stride, row_offset, state, dig, first, last):
    torch, abi, prover = gpu
    abi.check(prover.lib.pw_merkle_leaf_absorb(m_ptr, col_stride, cols_ptr, n_cols, pos0, height, row_stride, row_offset, state.data_ptr(),
                                               dig.data_ptr(), int(first), int(last)), "pw_merkle_leaf_absorb")
    torch.cuda.synchronize()


def absorb_level(gpu, rng, height, runs, dig=None):
    """The digests [height, 8] (canonical) of a level hashed run by run. runs: [(rows [height, w], form)], form = ("matrix", pad: the
    column stride is height + pad) | ("table",) | ("streamed", b: one launch per row offset r < 2^b, shuffled, on the matrix of the
    rows r + 2^b i). The rate position is carried as the callers carry it (segment_prover.hip commit_mixed). On the way: the digests
    hold the sentinel until the last run; a launch for one offset leaves the states and digests of all other rows as they were; the
    last run writes no state. The parked state words themselves are never compared with anything but their own earlier value."""
    torch, abi, prover = gpu
    state = sentinel(torch, height * 16)
    if dig is None:
        dig = sentinel(torch, height * 8)
    assert (raw(dig) == SENT).all()
    pos = 0
    for i, (rows, form) in enumerate(runs):
        first, last = i == 0, i + 1 == len(runs)
        w = rows.shape[1]
        assert rows.shape[0] == height and w >= 1
        run_start_s = before_s = raw(state).reshape(height, 16)
        before_d = raw(dig).reshape(height, 8)
        if form[0] == "streamed":
            stride = 1 << form[1]
            for r in rng.permutation(stride).tolist():
                sub = rows[r::stride]
                cs = len(sub) + int(rng.integers(0, 3))
                d_m = matrix_form(torch, rng, sub, cs)
                absorb(gpu, d_m.data_ptr(), cs, None, w, pos, len(sub), stride, r, state, dig, first, last)
                after_s, after_d = raw(state).reshape(height, 16), raw(dig).reshape(height, 8)
                others = np.arange(height) % stride != r
                assert (after_s[others] == before_s[others]).all() and (after_d[others] == before_d[others]).all(), (i, form, r)
                before_s, before_d = after_s, after_d
        elif form[0] == "matrix":
            d_m = matrix_form(torch, rng, rows, height + form[1])
            absorb(gpu, d_m.data_ptr(), height + form[1], None, w, pos, height, 1, 0, state, dig, first, last)
        else:
            d_m, d_ptrs = table_form(torch, rng, rows)
            absorb(gpu, None, 0, d_ptrs.data_ptr(), w, pos, height, 1, 0, state, dig, first, last)
        if last:
            assert (raw(state).reshape(height, 16) == run_start_s).all(), (i, form)
        else:
            assert (raw(dig) == SENT).all(), (i, form)
        pos = (pos + w) & 7
    return canonical(raw(dig)).reshape(height, 8)


ABSORB_HEIGHT = 257  # one workgroup is 256 rows


@functools.lru_cache(maxsize=None)
def absorb_case(pos0, n_cols):
    """(the widths of the runs, the level's rows, the reference digests) of the case: for pos0 > 0 a first run of pos0 or pos0 + 8
    columns (alternating by case) carries the rate position in; a closing run of 0 or 3 columns follows the run under test. Computed
    once (placeholder constants), shared by the forms and the POWDR_HASH_WAVES settings."""
    case = pos0 * 17 + n_cols - 1
    lead = 0 if pos0 == 0 else pos0 + 8 * (case & 1)
    close = 3 * (((n_cols - 1) // 2 + pos0) & 1)
    widths = [w for w in (lead, n_cols, close) if w]
    rows = np.random.default_rng(case).integers(0, P, (ABSORB_HEIGHT, sum(widths)), dtype=np.uint32)
    rows.setflags(write=False)
    want = ref.sponge(rows, constants())
    want.setflags(write=False)
    return widths, rows, want


def split(rows, widths):
    cuts = np.cumsum([0] + list(widths))
    return [rows[:, cuts[i]:cuts[i + 1]] for i in range(len(widths))]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["matrix", "table"])
def test_absorb_every_position_against_every_width(gpu, waves, form):
    """pw_merkle_leaf_absorb (leaf_absorb_kernel): every rate position carried in (0..7) against every width of the run (1..17), 257
    rows, all runs matrices (column stride height + 1) or all runs column-pointer tables: the digests equal the sponge over the
    concatenated rows"""
    rng = np.random.default_rng(77)
    for pos0 in range(8):
        for n_cols in range(1, 18):
            widths, rows, want = absorb_case(pos0, n_cols)
            assert ((widths[0] if pos0 else 0) & 7) == pos0  # the columns in front of the run under test
            f = ("matrix", 1) if form == "matrix" else ("table",)
            got = absorb_level(gpu, rng, ABSORB_HEIGHT, [(r, f) for r in split(rows, widths)])
            assert (got == want).all(), (pos0, n_cols, widths)


# ---- c. chains ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_case(name):
    """(level height, widths, forms, rows, reference digests) of a chain; computed once"""
    if name == "twenty_single_columns":  # the block stays open across eight launches, two and a half times over
        height, widths = ABSORB_HEIGHT, [1] * 20
        forms = [("matrix", i % 3) if i % 2 else ("table",) for i in range(20)]
        seed = 1
    elif name == "all_streamed":
        height, widths = 512, [3, 8, 1, 13, 5, 10]
        forms = [("streamed", b) for b in (3, 1, 2, 3, 1, 2)]
        seed = 2
    else:  # a seeded random partition of W <= 40 columns; every run a matrix, a table or streamed
        rng = np.random.default_rng(1000 + name)
        B = int(rng.integers(1, 4))
        height = 64 << B
        W = int(rng.integers(1, 41))
        n_runs = int(rng.integers(1, min(W, 9) + 1))
        cuts = np.sort(rng.choice(np.arange(1, W), n_runs - 1, replace=False)) if n_runs > 1 else np.zeros(0, np.int64)
        widths = np.diff(np.concatenate([[0], cuts, [W]])).astype(int).tolist()
        forms = []
        for _ in widths:
            kind = int(rng.integers(0, 3))
            forms.append(("matrix", int(rng.integers(0, 3))) if kind == 0 else ("table",) if kind == 1 else ("streamed", int(rng.integers(1, B + 1))))
        seed = 2000 + name
    assert all(w >= 1 for w in widths) and sum(widths) <= 40
    rows = np.random.default_rng(seed).integers(0, P, (height, sum(widths)), dtype=np.uint32)
    rows.setflags(write=False)
    want = ref.sponge(rows, constants())
    want.setflags(write=False)
    return height, widths, forms, rows, want


def check_chain(gpu, name):
    height, widths, forms, rows, want = chain_case(name)
    got = absorb_level(gpu, np.random.default_rng(5), height, list(zip(split(rows, widths), forms)))
    assert (got == want).all(), (name, height, widths, forms)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["twenty_single_columns", "all_streamed"])
def test_absorb_chain(gpu, waves, name):
    """twenty runs of one column each (matrices and tables alternating); a level whose every run is streamed (2, 4 or 8 row offsets
    per run, shuffled, all with the same pos0 / first / last)"""
    check_chain(gpu, name)


@pytest.mark.gpu
@pytest.mark.parametrize("group", range(5))
def test_absorb_random_partitions(gpu, waves, group):
    """50 seeded random partitions (ten per case) of W <= 40 columns into runs, each run randomly a matrix, a pointer table or a
    streamed matrix with row stride 2^b, b in 1..3, on a level of 2^B * 64 rows"""
    kinds = set()
    for seed in range(10 * group, 10 * group + 10):
        check_chain(gpu, seed)
        kinds |= {f[0] for f in chain_case(seed)[2]}
    assert kinds == {"matrix", "table", "streamed"}


# ---- d. the mixed tree ---------------------------------------------------------------------------------------------------------------
class MixedCase:
    """levels: {log height: [matrices [2^k, w] canonical, AIR order]}; every matrix is a device buffer of its own (column stride 2^k +
    a pad), the pointer table lists level L's columns first, level 0's last"""

    def __init__(self, gpu, levels, L, seed):
        torch, abi, prover = gpu
        self.gpu, self.levels, self.L = gpu, levels, L
        rng = np.random.default_rng(seed)
        self.keep, ptrs = [], []
        self.n_cols = np.zeros(L + 1, np.uint32)
        for k in range(L, -1, -1):
            for m in levels.get(k, []):
                assert m.shape[0] == 1 << k
                cs = (1 << k) + int(rng.integers(0, 4))
                d = matrix_form(torch, rng, m, cs)
                self.keep.append(d)
                ptrs += [d.data_ptr() + c * cs * 4 for c in range(m.shape[1])]
                self.n_cols[k] += m.shape[1]
        self.d_ptrs = torch.tensor(ptrs, dtype=torch.int64, device="cuda")
        self.tree_words = ((2 << L) - 1) * 8

    def commit(self, external=(), pass_cols=True, pass_inject=True):
        """all words of the tree (raw), after checking the sentinels: the words behind the tree, and in d_inject the words below level 0's
        slice and the slices of the levels that hold no matrix. External levels are hashed run by run (one run per matrix, the forms
        alternating) into their place first."""
        torch, abi, prover = self.gpu
        L = self.L
        rng = np.random.default_rng(9)
        d_dig = sentinel(torch, self.tree_words + 64)
        d_inj = sentinel(torch, (1 << L) * 8)
        ext = np.zeros(L + 1, np.uint32)
        for k in external:
            ext[k] = 1
            forms = [("table",), ("matrix", 2), ("streamed", 1) if k >= 1 else ("table",)]  # a single row has no second offset
            runs = [(m, forms[(i + k) % 3]) for i, m in enumerate(self.levels[k])]
            place = d_dig[:(1 << L) * 8] if k == L else d_inj[(1 << k) * 8:(2 << k) * 8]
            absorb_level(self.gpu, rng, 1 << k, runs, dig=place)
        abi.check(prover.lib.pw_merkle_commit_mixed(self.d_ptrs.data_ptr() if pass_cols else None, self.n_cols.ctypes.data, ext.ctypes.data, L,
                                                    d_dig.data_ptr(), d_inj.data_ptr() if pass_inject else None), "pw_merkle_commit_mixed")
        torch.cuda.synchronize()
        got, inj = raw(d_dig), raw(d_inj)
        assert (got[self.tree_words:] == SENT).all()
        assert (inj[:8] == SENT).all()
        for k in range(L):
            assert (inj[(1 << k) * 8:(2 << k) * 8] == SENT).all() == (k not in self.levels), k
        return got[:self.tree_words]


def random_levels(widths_by_log, seed):
    rng = np.random.default_rng(seed)
    return {k: [rng.integers(0, P, (1 << k, w), dtype=np.uint32) for w in ws] for k, ws in widths_by_log.items()}


CYCLE = [1, 8, 9, 3, 16, 23]
MIXED = {
    "single_row": (0, {0: [5]}),
    # thirteen populated levels in one launch; the widths repeat after six levels: 1 is held by three levels, every other by two (ties)
    "thirteen_levels": (12, {12 - i: [CYCLE[i % 6]] for i in range(13)}),
    "levels_10_7_0": (10, {10: [9], 7: [17], 0: [2]}),
    "three_matrices": (9, {9: [5, 8, 4], 3: [1, 7], 1: [3]}),
}


@functools.lru_cache(maxsize=None)
def mixed_case(name):
    L, widths = MIXED[name]
    levels = random_levels(widths, seed=len(name))
    mats = [m for lg in range(L, -1, -1) for m in levels.get(lg, [])]
    want = ref.mixed_tree(mats, constants())
    want.setflags(write=False)
    return L, levels, want


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MIXED))
def test_mixed_tree_all_words(gpu, waves, name):
    """pw_merkle_commit_mixed (leaf_hash_levels_kernel + compress_strided_kernel), every word of every level against the reference:
    L = 0; thirteen populated levels with ties in the widest-first order; populated levels 10, 7 and 0 only; a level of three matrices"""
    L, levels, want = mixed_case(name)
    case = MixedCase(gpu, levels, L, seed=3)
    got = case.commit(pass_inject=L > 0)
    assert (canonical(got) == want).all(), np.flatnonzero(canonical(got) != want)[:4]


@pytest.mark.gpu
@pytest.mark.parametrize("name,external", [("three_matrices", (9,)), ("three_matrices", (3, 1)), ("three_matrices", (9, 3, 1)),
                                           ("levels_10_7_0", (10, 0)), ("levels_10_7_0", (7,)), ("single_row", (0,))])
def test_mixed_tree_with_external_levels(gpu, waves, name, external):
    """the levels named `external` (the top level among them) hashed run by run with pw_merkle_leaf_absorb into their place and passed
    as external: the tree equals the all-resident call's and the reference; with every populated level external no leaf launch happens
    at all (and no column table is passed)"""
    L, levels, want = mixed_case(name)
    case = MixedCase(gpu, levels, L, seed=4)
    resident = case.commit(pass_inject=L > 0)
    got = case.commit(external=external, pass_cols=set(external) != set(levels), pass_inject=L > 0)
    assert (got == resident).all()
    assert (canonical(got) == want).all()


# ---- e. the binary tree around its tail boundary ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("height", [2048, 4096, 8192, 1 << 14])
def test_merkle_commit_around_the_tail_boundary(gpu, height):
    """pw_merkle_commit where compress_kernel hands over to compress_tail_kernel (kTailNodes = 2048): no, one, two and three launches
    of the former"""
    torch, abi, prover = gpu
    k = constants()
    rng = np.random.default_rng(height)
    for width in (1, 9):
        rows = rng.integers(0, P, (height, width), dtype=np.uint32)
        want = ref.binary_tree(ref.sponge(rows, k), k)
        d_m = matrix_form(torch, rng, rows, height)
        d_d = sentinel(torch, (2 * height - 1) * 8 + 64)
        abi.check(prover.lib.pw_merkle_commit(d_m.data_ptr(), height, width, d_d.data_ptr()), "pw_merkle_commit")
        torch.cuda.synchronize()
        got = raw(d_d)
        assert (got[len(want):] == SENT).all()
        assert (canonical(got[:len(want)]) == want).all(), width


@pytest.mark.gpu
@pytest.mark.parametrize("half", [1, 2, 1024, 4096])
def test_commit_ext_pairs(gpu, half):
    """pw_merkle_commit_ext_pairs (ext_pair_leaf_kernel + the binary tree): the FRI leaves and every inner node"""
    torch, abi, prover = gpu
    k = constants()
    v = np.random.default_rng(half).integers(0, P, (2 * half, 4), dtype=np.uint32)
    v[0], v[-1] = P - 1, 0
    want = ref.binary_tree(ref.ext_pair_leaves(v, k), k)
    d_v = to_dev(torch, v)
    d_d = sentinel(torch, (2 * half - 1) * 8 + 64)
    abi.check(prover.lib.pw_merkle_commit_ext_pairs(d_v.data_ptr(), half, d_d.data_ptr()), "pw_merkle_commit_ext_pairs")
    torch.cuda.synchronize()
    got = raw(d_d)
    assert (got[len(want):] == SENT).all()
    assert (canonical(got[:len(want)]) == want).all()


# ---- f. edge words through the parked states ---------------------------------------------------------------------------------------------
def check_edge_words(gpu):
    k = constants()
    H, W = 256, 17
    rng = np.random.default_rng(6)
    for kind, m in tables.edge_matrices(H, W).items():
        if kind == "random":
            continue
        rows = np.ascontiguousarray(m.reshape(W, H).T)
        want = ref.sponge(rows, k)
        for s in range(1, W):  # the first run leaves the block open at every position 1..7, closes it (8, 16), and passes it (9..15)
            forms = [("matrix", s % 3), ("table",)] if s & 1 else [("table",), ("matrix", s % 3)]
            got = absorb_level(gpu, rng, H, list(zip(split(rows, [s, W - s]), forms)))
            assert (got == want).all(), (kind, s)
        case = MixedCase(gpu, {8: [rows]}, 8, seed=7)
        assert (canonical(case.commit()) == ref.mixed_tree([rows], k)).all(), kind


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["placeholder"] + GPU_TABLES)
def test_edge_words_through_the_parked_states(gpu, waves, name):
    """zeros, p - 1, the two halves by column and one-hot rows, 17 columns x 256 rows, hashed through pw_merkle_leaf_absorb split into
    two runs at every one of the 16 positions — the only form in which such words leave the registers between two permutations, as
    the unreduced representatives permute<true> leaves — and through pw_merkle_commit_mixed as a single level; under the placeholder
    and under the tables that drive Poseidon2's signed ranges to their edges"""
    if name == "placeholder":
        check_edge_words(gpu)
        return
    with installed(name):
        check_edge_words(gpu)


# ---- the refusals --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_stage_entry_points_refuse_malformed_arguments(gpu):
    """every refusal the entry points document: a return code, and nothing written (the buffers still hold the sentinel afterwards).
    Needs a GPU only because the library does."""
    torch, abi, prover = gpu
    lib = prover.lib
    H, W = 8, 3
    rng = np.random.default_rng(0)
    rows = rng.integers(0, P, (H, W), dtype=np.uint32)
    d_m = matrix_form(torch, rng, rows, H)
    _, d_ptrs = keep = table_form(torch, rng, rows)
    d_d, d_s, d_i = sentinel(torch, 2 * H * 8 + 8), sentinel(torch, H * 16 + 8), sentinel(torch, H * 8)
    m, c, d, s, inj = d_m.data_ptr(), d_ptrs.data_ptr(), d_d.data_ptr(), d_s.data_ptr(), d_i.data_ptr()
    INVALID = 1  # hipErrorInvalidValue

    hash_bad = [(None, H, W, H, d, 1, 0), (m, H, W, H, None, 1, 0), (m, 0, W, H, d, 1, 0), (m, H, 0, H, d, 1, 0), (m, H, W, H - 1, d, 1, 0),
                (m, H, W, H, d, 0, 0), (m, H, W, H, d, 1, 1), (m, H, W, H, d, 2, 2)]
    for args in hash_bad:
        assert lib.pw_merkle_leaf_hash(*args) == -1, args
    assert lib.pw_merkle_leaf_hash(m, H, W, H, d + 4, 1, 0) == INVALID

    ok = dict(m=m, cs=H, cols=None, n=W, pos0=0, h=H, rs=1, ro=0, st=s, dg=d, first=1, last=1)

    def absorb_rc(**kw):
        a = {**ok, **kw}
        return lib.pw_merkle_leaf_absorb(a["m"], a["cs"], a["cols"], a["n"], a["pos0"], a["h"], a["rs"], a["ro"], a["st"], a["dg"], a["first"], a["last"])

    absorb_bad = [dict(m=None), dict(cols=c), dict(n=0), dict(h=0), dict(pos0=8, first=0), dict(pos0=3), dict(cs=H - 1), dict(rs=0), dict(rs=1, ro=1),
                  dict(rs=2, ro=2), dict(dg=None), dict(st=None, last=0), dict(st=None, first=0), dict(m=None, cols=c, n=0)]
    for kw in absorb_bad:
        assert absorb_rc(**kw) == -1, kw
    assert absorb_rc(dg=d + 4) == INVALID and absorb_rc(st=s + 8, last=0) == INVALID and absorb_rc(st=s + 4, first=0) == INVALID

    L = 3
    n_cols, none, ext_top = np.array([0, 0, 0, W], np.uint32), np.zeros(4, np.uint32), np.array([0, 0, 0, 1], np.uint32)
    below, ext_below = np.array([0, 1, 0, W], np.uint32), np.array([1, 0, 0, 1], np.uint32)
    p = lambda a: a.ctypes.data
    mixed_bad = [(c, None, p(none), L, d, inj), (c, p(n_cols), None, L, d, inj), (c, p(n_cols), p(none), L, None, inj),
                 (None, p(n_cols), p(none), L, d, inj),        # a resident level and no column table
                 (c, p(none), p(none), L, d, inj),             # a top level that is neither populated nor external
                 (c, p(below), p(none), L, d, None),           # a populated level below the top and no d_inject
                 (None, p(none), p(ext_below), L, d, None),    # an external one
                 (c, p(n_cols), p(none), 28, d, inj)]
    for args in mixed_bad:
        assert lib.pw_merkle_commit_mixed(*args) == -1, args
    assert lib.pw_merkle_commit_mixed(c, p(n_cols), p(none), L, d + 4, inj) == INVALID
    assert lib.pw_merkle_commit_mixed(c, p(n_cols), p(none), L, d, inj + 8) == INVALID

    d_v = to_dev(torch, rng.integers(0, P, (2 * H, 4), dtype=np.uint32))
    for args in [(None, H, d), (d_v.data_ptr(), H, None), (d_v.data_ptr(), 0, d), (d_v.data_ptr(), 3, d), (d_v.data_ptr(), 6, d)]:
        assert lib.pw_merkle_commit_ext_pairs(*args) == -1, args
    assert lib.pw_merkle_commit_ext_pairs(d_v.data_ptr(), H, d + 4) == INVALID

    torch.cuda.synchronize()
    assert (raw(d_d) == SENT).all() and (raw(d_s) == SENT).all() and (raw(d_i) == SENT).all()
    # the same buffers take the well-formed calls: a top level that is external and nothing else (no launch at all needs no table)
    k = constants()
    abi.check(absorb_rc(), "pw_merkle_leaf_absorb")
    abi.check(lib.pw_merkle_commit_mixed(None, p(none), p(ext_top), L, d, None), "pw_merkle_commit_mixed")
    torch.cuda.synchronize()
    assert (canonical(raw(d_d)[:(2 * H - 1) * 8]) == ref.mixed_tree([rows], k)).all()
    assert (raw(d_d)[(2 * H - 1) * 8:] == SENT).all() and (raw(d_s) == SENT).all()
    del keep
