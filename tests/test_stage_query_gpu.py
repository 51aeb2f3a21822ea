"""The end of a proof, kernel by kernel through the pw_stage_ entry points of the query phase (include/powdr_prover.h): pow_kernel /
pow_grind, gather_rows_kernel, gather_rows_multi_kernel, gather_words_kernel, canonicalize_kernel, gather_records_kernel,
ext_to_cols_kernel, and the query pass of a streamed proof — streamed::query_rows over subcoset_query_rows in both forms
(select_xpow_kernel, the SELECT mode of ntt_group_kernel, select_reduce_kernel / select_finish_kernel) and over the fall-back
subcoset_lde_first_group + subcoset_rows_kernel. Every comparison is equality of every word; every output buffer starts as the sentinel
and the words a call must not write still hold it afterwards.

References: a witness is the oracle's or_pow_witness (the oracle's own Challenger: copy, observe, sample_bits), which
tests/test_stage_ref_cpu.py holds to a numpy search; a row of the extension is sum_k c_k x^k straight from the coefficients
(tests/_stage_ref.lde_rows, held to the oracle's LDE there), so no transform of the code under test prepares an input; the gathers are
numpy indexing.

Query rows, shape (log_h, log_blocks) -> the form every sub-coset with a query must report (FORMS; 1 = one pass with stored terms,
2 = one pass with 64-bit atomic sums, 3 = partial transform + subcoset_rows): the one-pass forms exist from 2^14-row sub-cosets on and
for log_blocks <= 2. Each case runs under POWDR_QUERY_SELECT unset, 2 and 0; the offered scratch is swept across the two thresholds
the header states.

Left out: a width above 65 535. The one-pass form declines it (blockIdx.y is the column) — at the smallest qualifying height, 2^14
rows, that is 4 GiB of coefficients and as much scratch for the partial transform."""
import ctypes as C

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _edge_values as ev
from tests import _stage_ref as ref
from tests.test_poseidon2_edge_tables import installed
from tests.test_prover_gpu import gpu  # noqa: F401  (the module-level fixture: torch, abi, prover — or a skip without a GPU)
from tests.test_stage_kernels_gpu import SENT, raw, raw_dev, sentinel, to_dev

P = om.P
INVALID = 1  # hipErrorInvalidValue


# ---- grinding ----------------------------------------------------------------------------------------------------------------------
def grind(abi, lib, state, pending, bits):
    state, pending = np.ascontiguousarray(state, np.uint32), np.ascontiguousarray(pending, np.uint32)
    w = C.c_uint32(SENT)
    abi.check(lib.pw_stage_pow_grind(state.ctypes.data, pending.ctypes.data if len(pending) else None, len(pending), bits, C.byref(w)),
              "pw_stage_pow_grind")
    return w.value


def check_grinding(abi, lib, families):
    for name in families:
        state, pending = ref.pow_families(np.random.default_rng(400))[name]
        for in_len in range(8):
            for bits in (1, 4, 8, 12):
                want = sm.pow_witness(state, pending[:in_len], bits, 0, 1 << 20)
                assert want != sm.POW_NONE  # (2^20 candidates at 12 bits: a miss has probability e^-256)
                assert grind(abi, lib, state, pending[:in_len], bits) == want, (name, in_len, bits)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["random", "zero", "pm1", "edge"])
def test_the_witness_is_the_smallest_for_every_pending_count(gpu, family):
    """in_len 0 .. 7 (at 7 the witness fills the rate and observe() permutes, below a sample does) x bits 1, 4, 8, 12: the SMALLEST
    witness of a real observe-then-sample transcript"""
    torch, abi, prover = gpu
    check_grinding(abi, prover.lib, [family])


@pytest.mark.gpu
def test_the_witness_under_an_edge_constant_table(gpu):
    """the random states once more with every folded round constant at +(p - 1) / 2, in the library and in the oracle"""
    torch, abi, prover = gpu
    with installed("plus_half"):
        check_grinding(abi, prover.lib, ["random"])


def crossing_case(seed, in_len):
    rng = np.random.default_rng([300, seed])
    return rng.integers(0, P, 16, dtype=np.uint32), rng.integers(0, P, 7, dtype=np.uint32)[:in_len]


# (seed, in_len, the first witness at 21 bits, the batches of 2^20 candidates that hold none): found with or_pow_witness on the CPU
CROSSINGS = [(0, 7, 1625126, 1), (10, 3, 2198328, 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,in_len,witness,batches", CROSSINGS)
def test_the_search_goes_on_into_the_next_batches(gpu, seed, in_len, witness, batches):
    """21 bits: the first witness lies behind the first 2^20 candidates (behind the first 2^21), so pow_kernel runs with base != 0 and
    pow_grind's loop carries `best` from batch to batch"""
    torch, abi, prover = gpu
    state, pending = crossing_case(seed, in_len)
    want = sm.pow_witness(state, pending, 21, 0, 1 << 22)
    assert want == witness and want >> 20 >= batches, (want, witness)  # a changed seed fails here, not silently in the first batch
    assert grind(abi, prover.lib, state, pending, 21) == want


# ---- query rows --------------------------------------------------------------------------------------------------------------------
FORMS = {(1, 1): 3, (3, 1): 3, (3, 2): 3, (13, 1): 3, (14, 1): 1, (15, 2): 1, (16, 3): 3, (16, 1): 1}
QUALIFYING = [s for s, f in FORMS.items() if f == 1]
MODES = [None, "2", "0"]  # POWDR_QUERY_SELECT


def ev2(x):
    return (x + 1) & ~1


def select_need(cols, n_r, tiles):
    """the header's formula: (words the atomic form needs, words the stored-terms form needs) for n_r queries in a sub-coset of
    `tiles` 2^12-row tiles"""
    a = (1 << 13) + ev2(n_r) + ev2(n_r * tiles) + 2 * cols * n_r
    return a, a + cols * tiles * n_r


def coefficients(family, rng, cols, H):
    if family == "random":
        return rng.integers(0, P, (cols, H), dtype=np.uint32)
    if family == "pm1":
        return np.full((cols, H), P - 1, np.uint32)
    if family == "edge":
        return ev.EDGE[rng.integers(0, len(ev.EDGE), (cols, H))]
    c = np.zeros((cols, H), np.uint32)  # "single": all 0 except one coefficient a column — the last, the first, a random one
    for col in range(cols):
        c[col, [H - 1, 0, int(rng.integers(0, H))][col % 3]] = [P - 1, 1, int(rng.integers(1, P))][col % 3]
    return c


def row_of(local, r, b):
    return (local << b) | r


def index_lists(rng, log_h, b):
    """name -> query indices into the 2^(log_h + 1) rows; sub-coset of j = j mod 2^b, its row there j >> b"""
    N, nb, m = 2 << log_h, 1 << b, (2 << log_h) >> b
    pick = lambda n, r: [row_of(int(i), r, b) for i in rng.choice(m, size=min(n, m), replace=False)]
    out = {"row0": [0], "last": [N - 1], "one_subcoset": pick(5, nb - 1), "odd": [int(j) for j in rng.integers(0, N, 7)],
           "descending": sorted((int(j) for j in rng.integers(0, N, 9)), reverse=True)}
    a, bb, c, d = (int(j) for j in rng.integers(0, N, 4))
    out["repeat"] = [a, bb, a, c, d, a]
    # the 128-lane edge of select_reduce_kernel, per sub-coset: 127 in the first and 128 in the second; 129 in the last and 1 in the first
    e1, e2 = pick(127, 0) + pick(128, 1 % nb), pick(129, nb - 1) + pick(1, 0)
    out["count127_128"] = [e1[k] for k in rng.permutation(len(e1))]
    out["count129"] = [e2[k] for k in rng.permutation(len(e2))]
    if m > 4096:  # the same position inside a tile, another tile
        i = int(rng.integers(0, m - 4096))
        out["tile_pairs"] = [row_of(i, 0, b), row_of(i + 4096, 0, b), row_of(m - 1 - 4096, nb - 1, b), row_of(m - 1, nb - 1, b)]
    return out


def mixed_list(rng, log_h, b):
    """row 0, the last row, a repeat at non-adjacent positions, a tile pair, random rows: 9 queries (odd)"""
    N, m = 2 << log_h, (2 << log_h) >> b
    a, c = (int(j) for j in rng.integers(0, N, 2))
    pair = [row_of(5, 0, b), row_of(5 + 4096, 0, b)] if m > 4096 else [1 % N, (N - 2) % N]
    return [a, 0, pair[0], a, N - 1, c, pair[1], a, 0]


class QueryRows:
    """one matrix of coefficients on the device and the buffers of pw_stage_query_rows"""

    def __init__(self, torch, abi, lib, c, log_h, b, max_queries):
        self.torch, self.abi, self.lib, self.c, self.log_h, self.b = torch, abi, lib, c, log_h, b
        self.cols, self.m = len(c), (2 << log_h) >> b
        self.tiles = max(self.m >> 12, 1)
        self.arrays = ref.coefficient_arrays(c, log_h)
        self.d_coef = to_dev(torch, self.arrays)
        self.coef_words = raw(torch, self.d_coef).copy()
        self.work_words = max(self.cols * self.m, select_need(self.cols, max_queries, self.tiles)[1])
        self.d_work = sentinel(torch, self.work_words + 64)
        self.d_scale = sentinel(torch, (1 << 13) + 64)

    def run(self, idx, select_words=None, monkeypatch=None, mode=None):
        """-> (rows as canonical values, forms per sub-coset); the raw words are below p, the tails still hold the sentinel"""
        torch = self.torch
        if monkeypatch is not None:
            monkeypatch.delenv("POWDR_QUERY_SELECT", raising=False)
            if mode is not None:
                monkeypatch.setenv("POWDR_QUERY_SELECT", mode)
        h_idx = np.ascontiguousarray(idx, np.uint32)
        n = len(h_idx)
        d_rows = sentinel(torch, n * self.cols + 64)
        forms = np.full((1 << self.b) + 8, 0xEE, np.uint8)
        rc = self.lib.pw_stage_query_rows(self.d_coef.data_ptr(), self.cols, self.log_h, self.b, h_idx.ctypes.data, n, self.d_work.data_ptr(),
                                          self.work_words, self.work_words if select_words is None else select_words, self.d_scale.data_ptr(),
                                          d_rows.data_ptr(), forms.ctypes.data)
        self.abi.check(rc, "pw_stage_query_rows")
        words = raw(torch, d_rows)
        assert (words[n * self.cols:] == SENT).all() and (forms[1 << self.b:] == 0xEE).all()
        assert (raw(torch, self.d_work)[self.work_words:] == SENT).all() and (raw(torch, self.d_scale)[1 << 13:] == SENT).all()
        assert (words[:n * self.cols] < P).all()
        return om.from_monty(words[:n * self.cols]).reshape(n, self.cols), forms[:1 << self.b].tolist()

    def check(self, idx, monkeypatch, form, tag):
        want = ref.lde_rows(self.c, self.log_h, idx)
        counts = np.bincount(np.asarray(idx) & ((1 << self.b) - 1), minlength=1 << self.b)
        for mode in MODES:
            got, forms = self.run(idx, monkeypatch=monkeypatch, mode=mode)
            expect = 3 if (form == 3 or mode == "0") else 2 if mode == "2" else 1
            assert forms == [expect if n_r else 0 for n_r in counts], (tag, mode, forms)
            assert (got == want).all(), (tag, mode, np.argwhere(got != want)[:4].tolist())
        assert (raw(self.torch, self.d_coef) == self.coef_words).all(), tag  # the coefficients are read, never written


@pytest.mark.gpu
@pytest.mark.parametrize("log_h,b", list(FORMS), ids=[f"{s[0]}-{s[1]}" for s in FORMS])
def test_query_rows_for_every_index_list(gpu, monkeypatch, log_h, b):
    """3 random columns; row 0, the last row, one sub-coset alone, repeats, 127 / 128 / 129 queries in a sub-coset, an odd count,
    descending order, pairs at one position of two tiles — in all three modes, with the predicted form per sub-coset"""
    torch, abi, prover = gpu
    rng = np.random.default_rng([500, log_h, b])
    q = QueryRows(torch, abi, prover.lib, coefficients("random", rng, 3, 1 << log_h), log_h, b, 256)
    for name, idx in index_lists(rng, log_h, b).items():
        q.check(idx, monkeypatch, FORMS[(log_h, b)], name)


@pytest.mark.gpu
@pytest.mark.parametrize("cols", [1, 257])
@pytest.mark.parametrize("log_h,b", list(FORMS), ids=[f"{s[0]}-{s[1]}" for s in FORMS])
def test_query_rows_at_one_column_and_past_a_block_of_columns(gpu, monkeypatch, log_h, b, cols):
    """width 1, and 257: the second 256-column block of subcoset_rows_kernel / select_finish_kernel holds one column"""
    torch, abi, prover = gpu
    rng = np.random.default_rng([501, log_h, b, cols])
    q = QueryRows(torch, abi, prover.lib, coefficients("random", rng, cols, 1 << log_h), log_h, b, 16)
    q.check(mixed_list(rng, log_h, b)[:9 if log_h < 16 or cols == 1 else 5], monkeypatch, FORMS[(log_h, b)], cols)


@pytest.mark.gpu
@pytest.mark.parametrize("family", ["pm1", "single", "edge"])
@pytest.mark.parametrize("log_h,b", list(FORMS), ids=[f"{s[0]}-{s[1]}" for s in FORMS])
def test_query_rows_of_edge_coefficients(gpu, monkeypatch, log_h, b, family):
    """every coefficient p - 1 (the folds and the sums at their largest), one non-zero coefficient a column (a row is one power of
    x), the edge words"""
    torch, abi, prover = gpu
    rng = np.random.default_rng([502, log_h, b, len(family)])
    q = QueryRows(torch, abi, prover.lib, coefficients(family, rng, 3, 1 << log_h), log_h, b, 16)
    q.check(mixed_list(rng, log_h, b), monkeypatch, FORMS[(log_h, b)], family)


@pytest.mark.gpu
@pytest.mark.parametrize("log_h,b", QUALIFYING, ids=[f"{s[0]}-{s[1]}" for s in QUALIFYING])
def test_query_rows_across_the_scratch_thresholds(gpu, monkeypatch, log_h, b):
    """the offered words swept across the two needs the header states: one word short of the atomic form's -> the partial transform;
    from there to one word short of the stored terms' -> atomic sums; from there on -> stored terms. The same rows every time."""
    torch, abi, prover = gpu
    rng = np.random.default_rng([503, log_h, b])
    cols = 3
    q = QueryRows(torch, abi, prover.lib, coefficients("random", rng, cols, 1 << log_h), log_h, b, 16)
    monkeypatch.delenv("POWDR_QUERY_SELECT", raising=False)
    seen = set()
    for n_r in (5, 6):  # an odd count: the 64-bit sums sit behind an odd number of words rounded up
        idx = [row_of(int(i), 0, b) for i in rng.choice(q.m, size=n_r, replace=False)]
        want = ref.lde_rows(q.c, log_h, idx)
        need2, need1 = select_need(cols, n_r, q.tiles)
        assert need2 < need1 <= q.work_words
        for offered, form in [(0, 3), (need2 - 1, 3), (need2, 2), (need1 - 1, 2), (need1, 1), (q.work_words, 1)]:
            got, forms = q.run(idx, select_words=offered)
            assert forms == [form] + [0] * ((1 << b) - 1), (n_r, offered, forms)
            assert (got == want).all(), (n_r, offered)
            seen.add(form)
    assert seen == {1, 2, 3}


# ---- the gathers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("height", [5, 512])
def test_gather_rows(gpu, height):
    """widths at the 256-column block edge, indices with row 0, the last row and repeats, one query and a hundred, raw and canonical"""
    torch, abi, prover = gpu
    rng = np.random.default_rng([600, height])
    for width in (1, 255, 256, 257, 600):
        m = rng.integers(0, P, (width, height), dtype=np.uint32)
        m[:, 0], m[:, -1] = ev.EDGE[rng.integers(0, len(ev.EDGE), width)], P - 1
        d_m = to_dev(torch, m)
        for n in (1, 100):
            idx = np.concatenate([[height - 1, 0, height - 1, 0], rng.integers(0, height, 96)]).astype(np.uint32)[:n]
            d_idx = raw_dev(torch, idx)
            want = ref.gather_rows(m, idx).reshape(-1)
            for canonical in (0, 1):
                d_o = sentinel(torch, n * width + 64)
                abi.check(prover.lib.pw_stage_gather_rows(d_m.data_ptr(), height, width, d_idx.data_ptr(), n, canonical, d_o.data_ptr()),
                          "pw_stage_gather_rows")
                got = raw(torch, d_o)
                assert (got[n * width:] == SENT).all(), (width, n, canonical)
                assert (got[:n * width] == (want if canonical else om.to_monty(want))).all(), (width, n, canonical)


@pytest.mark.gpu
@pytest.mark.parametrize("idx_offs", [[0, 7, 14, 21, 28], [0, 7, 14, 21, 7]], ids=["disjoint", "shared"])
def test_gather_rows_multi(gpu, idx_offs):
    """five jobs in one launch: widths 1 next to 600, 3, 2050 (past one sweep of the grid's 8 x 256 columns) and 257; heights 2^9, 8, 5,
    16, 64; every job its own range of the output, with gaps that must still hold the sentinel. `disjoint`: every job its own slice of
    the indices; `shared`: on purpose, the last job reads the second job's slice, as the trees of one AIR share theirs in a segment"""
    torch, abi, prover = gpu
    from powdr_amd.prover import PwStageGatherJob

    rng = np.random.default_rng(601)
    n, shapes = 7, [(1, 512), (600, 8), (3, 5), (2050, 16), (257, 64)]
    heights = [h for _, h in shapes]
    idx = np.zeros(35, np.uint32)
    for k, off in enumerate(idx_offs):
        h = min(hh for hh, o in zip(heights, idx_offs) if o == off)
        idx[off:off + n] = np.concatenate([[h - 1, 0, h - 1], rng.integers(0, h, n - 3)])
    mats = [rng.integers(0, P, s, dtype=np.uint32) for s in shapes]
    d_mats = [raw_dev(torch, m) for m in mats]
    jobs, want, out_off = (PwStageGatherJob * len(shapes))(), {}, 3
    for k, (w, h) in enumerate(shapes):
        jobs[k] = PwStageGatherJob(d_mats[k].data_ptr(), h, w, idx_offs[k], out_off)
        want[out_off] = ref.gather_rows(mats[k], idx[idx_offs[k]:idx_offs[k] + n]).reshape(-1)
        out_off += n * w + 5 + k
    d_idx, d_o = raw_dev(torch, idx), sentinel(torch, out_off + 64)
    abi.check(prover.lib.pw_stage_gather_rows_multi(jobs, len(shapes), d_idx.data_ptr(), n, d_o.data_ptr()), "pw_stage_gather_rows_multi")
    got = raw(torch, d_o)
    expect = np.full(out_off + 64, SENT, np.uint32)
    for off, rows in want.items():
        expect[off:off + len(rows)] = rows
    assert (got == expect).all(), np.argwhere(got != expect)[:8].tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("words", [8, 4])
def test_gather_records(gpu, words):
    """digests (8 words) and extension elements (4): counts around the 256-thread block for both sizes, repeated offsets, offsets at the
    arena's first and last record"""
    torch, abi, prover = gpu
    rng = np.random.default_rng([602, words])
    arena = rng.integers(0, 1 << 32, 4096, dtype=np.uint32)
    d_a = raw_dev(torch, arena)
    for n in (1, 32, 33, 64, 65):
        offs = np.concatenate([[4096 - words, 0, 4096 - words], rng.integers(0, 4096 // words, 64) * words]).astype(np.uint64)[:n]
        d_o = sentinel(torch, n * words + 64)
        abi.check(prover.lib.pw_stage_gather_records(d_a.data_ptr(), offs.ctypes.data, words, n, d_o.data_ptr()), "pw_stage_gather_records")
        got = raw(torch, d_o)
        assert (got[n * words:] == SENT).all() and (got[:n * words] == ref.gather_records(arena, offs, words).reshape(-1)).all(), n


@pytest.mark.gpu
def test_gather_words_canonicalize_and_ext_to_cols(gpu):
    torch, abi, prover = gpu
    lib = prover.lib
    rng = np.random.default_rng(603)
    pool = rng.integers(0, 1 << 32, 1000, dtype=np.uint32)
    d_pool = raw_dev(torch, pool)
    for n in (1, 256, 257):
        at = np.concatenate([[999, 0, 999], rng.integers(0, 1000, 254)])[:n]
        d_ptrs = raw_dev(torch, (d_pool.data_ptr() + 4 * at).astype(np.uint64))
        d_o = sentinel(torch, n + 64)
        abi.check(lib.pw_stage_gather_words(d_ptrs.data_ptr(), n, d_o.data_ptr()), "pw_stage_gather_words")
        got = raw(torch, d_o)
        assert (got[n:] == SENT).all() and (got[:n] == pool[at]).all(), n
    special = np.array([0, 1, P - 1, (1 << 32) % P], np.uint32)  # the words themselves: 2^32 mod p is the word of the value 1
    for n in (1, 256, 257):
        words = np.concatenate([special, rng.integers(0, P, 253, dtype=np.uint32)])[:n]
        d_w = torch.cat([raw_dev(torch, words), sentinel(torch, 64)])
        abi.check(lib.pw_stage_canonicalize(d_w.data_ptr(), n), "pw_stage_canonicalize")
        got = raw(torch, d_w)
        assert (got[n:] == SENT).all() and (got[:n] == ref.from_word(words)).all(), n
        assert n < 4 or int(got[3]) == 1
    for n in (1, 255, 256, 257):
        v = rng.integers(0, 1 << 32, (n, 4), dtype=np.uint32)
        d_v, d_o = raw_dev(torch, v), sentinel(torch, 4 * n + 64)
        abi.check(lib.pw_stage_ext_to_cols(d_v.data_ptr(), n, d_o.data_ptr()), "pw_stage_ext_to_cols")
        got = raw(torch, d_o)
        assert (got[4 * n:] == SENT).all() and (got[:4 * n] == ref.ext_to_cols(v).reshape(-1)).all(), n


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_malformed_arguments_are_refused_before_any_launch(gpu):
    """-1 for NULL pointers, zero sizes, logs out of range, words >= p, in_len > 7, bits outside 1 .. 31, more than 65 535 queries or jobs, a
    query index >= 2 H and a work area below cols * m (or below what is offered of it); hipErrorInvalidValue for the two alignments;
    the outputs still hold their sentinel afterwards, and a well-formed call of each succeeds"""
    torch, abi, prover = gpu
    from powdr_amd.prover import PwStageGatherJob

    lib = prover.lib
    rng = np.random.default_rng(650)
    d_m, d_o, d_x = raw_dev(torch, rng.integers(0, P, 4096, dtype=np.uint32)), sentinel(torch, 1024), sentinel(torch, (1 << 13) + 4096)
    d_i = raw_dev(torch, np.zeros(16, np.uint32))
    d_p = raw_dev(torch, np.full(4, d_m.data_ptr(), np.uint64))
    m, o, x, i, p = d_m.data_ptr(), d_o.data_ptr(), d_x.data_ptr(), d_i.data_ptr(), d_p.data_ptr()
    st, pend, big = np.zeros(16, np.uint32), np.zeros(8, np.uint32), np.full(16, P, np.uint32)
    s, q, bad = st.ctypes.data, pend.ctypes.data, big.ctypes.data
    w = C.c_uint32(SENT)
    offs = np.zeros(4, np.uint64)
    f = offs.ctypes.data
    jobs = (PwStageGatherJob * 2)(PwStageGatherJob(m, 8, 2, 0, 0), PwStageGatherJob(m, 8, 2, 0, 64))
    nullm = (PwStageGatherJob * 1)(PwStageGatherJob(None, 8, 2, 0, 0))
    zeroh = (PwStageGatherJob * 1)(PwStageGatherJob(m, 0, 2, 0, 0))
    zerow = (PwStageGatherJob * 1)(PwStageGatherJob(m, 8, 0, 0, 0))
    qi, far = np.array([0, 15, 3], np.uint32), np.array([0, 16, 3], np.uint32)  # log_h 3: 16 rows
    forms = np.full(8, 0xEE, np.uint8)
    g, gf, fm = qi.ctypes.data, far.ctypes.data, forms.ctypes.data
    refused = [
        lib.pw_stage_pow_grind(None, q, 3, 4, C.byref(w)), lib.pw_stage_pow_grind(s, None, 3, 4, C.byref(w)), lib.pw_stage_pow_grind(s, q, 8, 4, C.byref(w)),
        lib.pw_stage_pow_grind(s, q, 3, 0, C.byref(w)), lib.pw_stage_pow_grind(s, q, 3, 32, C.byref(w)), lib.pw_stage_pow_grind(bad, q, 3, 4, C.byref(w)),
        lib.pw_stage_pow_grind(s, bad, 3, 4, C.byref(w)), lib.pw_stage_pow_grind(s, q, 3, 4, None),
        lib.pw_stage_gather_rows(None, 8, 2, i, 3, 0, o), lib.pw_stage_gather_rows(m, 0, 2, i, 3, 0, o), lib.pw_stage_gather_rows(m, 8, 0, i, 3, 0, o),
        lib.pw_stage_gather_rows(m, 8, 2, None, 3, 0, o), lib.pw_stage_gather_rows(m, 8, 2, i, 0, 0, o), lib.pw_stage_gather_rows(m, 8, 2, i, 3, 1, None),
        lib.pw_stage_gather_rows(m, 8, 2, i, 65536, 0, o),
        lib.pw_stage_canonicalize(None, 4), lib.pw_stage_canonicalize(o, 0),
        lib.pw_stage_gather_rows_multi(None, 2, i, 3, o), lib.pw_stage_gather_rows_multi(jobs, 0, i, 3, o), lib.pw_stage_gather_rows_multi(jobs, 2, None, 3, o),
        lib.pw_stage_gather_rows_multi(jobs, 2, i, 0, o), lib.pw_stage_gather_rows_multi(jobs, 2, i, 3, None), lib.pw_stage_gather_rows_multi(nullm, 1, i, 3, o),
        lib.pw_stage_gather_rows_multi(zeroh, 1, i, 3, o), lib.pw_stage_gather_rows_multi(zerow, 1, i, 3, o), lib.pw_stage_gather_rows_multi(jobs, 2, i, 65536, o),
        lib.pw_stage_gather_rows_multi(jobs, 65536, i, 3, o), lib.pw_stage_query_rows(m, 2, 3, 1, g, 65536, x, 4096, 4096, x, o, fm),
        lib.pw_stage_gather_records(None, f, 8, 4, o), lib.pw_stage_gather_records(m, None, 8, 4, o), lib.pw_stage_gather_records(m, f, 0, 4, o),
        lib.pw_stage_gather_records(m, f, 8, 0, o), lib.pw_stage_gather_records(m, f, 8, 4, None),
        lib.pw_stage_gather_words(None, 4, o), lib.pw_stage_gather_words(p, 0, o), lib.pw_stage_gather_words(p, 4, None),
        lib.pw_stage_ext_to_cols(None, 4, o), lib.pw_stage_ext_to_cols(m, 0, o), lib.pw_stage_ext_to_cols(m, 4, None), lib.pw_stage_ext_to_cols(m, (1 << 27) + 1, o),
        lib.pw_stage_query_rows(None, 2, 3, 1, g, 3, x, 4096, 4096, x, o, fm), lib.pw_stage_query_rows(m, 0, 3, 1, g, 3, x, 4096, 4096, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 27, 1, g, 3, x, 4096, 4096, x, o, fm), lib.pw_stage_query_rows(m, 2, 3, 0, g, 3, x, 4096, 4096, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 3, 4, g, 3, x, 4096, 4096, x, o, fm), lib.pw_stage_query_rows(m, 2, 8, 6, g, 3, x, 4096, 4096, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 3, 1, None, 3, x, 4096, 4096, x, o, fm), lib.pw_stage_query_rows(m, 2, 3, 1, g, 0, x, 4096, 4096, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 3, 1, gf, 3, x, 4096, 4096, x, o, fm), lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, None, 4096, 4096, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x, 15, 15, x, o, fm), lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x, 16, 17, x, o, fm),
        lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x, 4096, 4096, None, o, fm), lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x, 4096, 4096, x, None, fm),
    ]
    assert refused == [-1] * len(refused), refused
    assert lib.pw_stage_query_rows(m + 4, 2, 3, 1, g, 3, x, 4096, 4096, x, o, fm) == INVALID  # (the staged loads take 16 bytes)
    assert lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x + 4, 4096, 4096, x, o, fm) == INVALID  # (the 64-bit sums)
    assert (raw(torch, d_o) == SENT).all() and (raw(torch, d_x) == SENT).all() and w.value == SENT and (forms == 0xEE).all()
    abi.check(lib.pw_stage_pow_grind(s, q, 3, 4, C.byref(w)), "pw_stage_pow_grind")
    assert w.value == sm.pow_witness(st, pend[:3], 4)
    abi.check(lib.pw_stage_gather_rows(m, 8, 2, i, 3, 1, o), "pw_stage_gather_rows")
    abi.check(lib.pw_stage_gather_rows_multi(jobs, 2, i, 3, o), "pw_stage_gather_rows_multi")
    abi.check(lib.pw_stage_gather_records(m, f, 8, 4, o), "pw_stage_gather_records")
    abi.check(lib.pw_stage_gather_words(p, 4, o), "pw_stage_gather_words")
    abi.check(lib.pw_stage_ext_to_cols(m, 4, o), "pw_stage_ext_to_cols")
    abi.check(lib.pw_stage_canonicalize(o, 4), "pw_stage_canonicalize")
    abi.check(lib.pw_stage_query_rows(m, 2, 3, 1, g, 3, x, 16, 16, x + 4 * 4096, o, None), "pw_stage_query_rows")
    torch.cuda.synchronize()
