"""The stage in front of tests/test_stage_kernels_gpu.py — the LogUp permutation trace and the quotient — kernel by kernel through the
pw_stage_ entry points that take a prover (include/powdr_prover.h), against tests/_stage_ref.py (tied down by
tests/test_stage_ref_cpu.py), on EVERY implementation: logup_perm_kernel<FAST>, quotient_logup_kernel<XBC, FAST, .> (also main_only),
quotient_kernel<XBC, .> with its chunks and quotient_combine_kernel, quotient_logup_tail_kernel, rowsum_combine_kernel, and the
run-time specialised pwj_perm_* / pwj_quotient_* kernels with one and with several chunks and units. Field arithmetic is exact: every
comparison is equality of every output word, and the words behind an output must still hold the sentinel they started with.

Four provers per AIR (PROVERS): `forms` (interpreter, small forms, xbc), `postfix` (POWDR_LOGUP_INTERPRET=1 POWDR_QUOTIENT_XBC=0),
`jit` (specialised), `jit-small` (POWDR_JIT_CHUNK_COST=200 POWDR_JIT_UNIT_CHUNKS=1: several chunks, one per unit).

Input families. `random`: canonical words. `edge`: cells and table coordinates from tests/_edge_values.EDGE. `bound_pos / _neg / _alt`
(the column AIR): every argument cell is the value whose device word is p - 1, every coordinate of blpow[1..] the word whose centred
value is +(p-1)/2 (-(p-1)/2; alternating along the argument index), alpha's coordinates the extreme of the first product's sign — a
table no transcript produces: seed and products of pwj::DenominatorAcc pile up to the budget its comment states; every second lane is
all-zero cells. For the quotient: apow all words p - 1, cells at word p - 1 (bb::ExtProductAcc / ExtWideAcc carry from the second
term on), permutation cells from EDGE."""
import ctypes as C

import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _edge_values as ev
from tests import _stage_ref as ref
from tests._edge_values import MUL, PA, PC, SUB, _programs
from tests.test_jit import hand_made_air
from tests.test_prover_gpu import gpu  # noqa: F401  (the module-level fixture: torch, abi, prover — or a skip without a GPU)
from tests.test_stage_kernels_gpu import ALL_PM1, SENT, ZERO4, h4, rand_ext, raw, raw_dev, scalar_set, sentinel, split, to_dev

P = om.P
HALF = (P - 1) // 2
PM1 = ev.word(P - 1)                                   # the canonical value whose device word is p - 1
WORD_HI, WORD_LO = ev.word(HALF), ev.word(HALF + 1)   # device words centred at +(p-1)/2 and -(p-1)/2
PROVERS = {
    "forms": {"POWDR_JIT": "0"},
    "postfix": {"POWDR_JIT": "0", "POWDR_LOGUP_INTERPRET": "1", "POWDR_QUOTIENT_XBC": "0"},
    "jit": {},
    "jit-small": {"POWDR_JIT_CHUNK_COST": "200", "POWDR_JIT_UNIT_CHUNKS": "1"},
}
_ENV = ["POWDR_JIT", "POWDR_LOGUP_INTERPRET", "POWDR_QUOTIENT_XBC", "POWDR_JIT_CHUNK_COST", "POWDR_JIT_UNIT_CHUNKS", "POWDR_JIT_MIN_LOG_HEIGHT"]
PERM_FAMILIES = {"hand": ["random", "edge"], "column": ["random", "edge", "bound_pos", "bound_neg", "bound_alt"]}
VANISH_ROWS = (0, 255, 256, 511)                       # row 0, lane 255, lane 256, the last row of 2^9


# ---- AIRs --------------------------------------------------------------------------------------------------------------------------
COLUMN_ARGS = [0, 1, 2, 3, 4, 5, 7, 1, 2, 3]   # arguments per interaction: groups (0 1 2) (3 4) (5 7) (1 2) (3)
COLUMN_BUSES = [2, 2, 3, 4, 4, 5, 6, 7, 7, 8]


def column_air():
    """Every constraint, multiplicity and argument a bare column, each with a column of its own. Five constraints; ten interactions with
    0 .. 5 and 7 arguments — every parity of DenominatorAcc's `pending` at result(), one, two and three reductions — in five groups of
    3, 2, 2, 2 and 1 members (an argument-less denominator has degree 0: it lets a third member in), so the specialised kernels' second
    batch of four groups holds a single group."""
    col = lambda c: [PA, c]
    nxt, interactions = 5, []
    for bus, n_args in zip(COLUMN_BUSES, COLUMN_ARGS):
        interactions.append((bus, col(nxt), [col(nxt + 1 + j) for j in range(n_args)]))
        nxt += 1 + n_args
    cons, it = _programs([col(c) for c in range(5)], interactions)
    return nxt, cons, it


def wide_air():
    """constraints only, 66 of them (products of two columns minus a third): quotient_chunks exceeds 1 at every height used here"""
    W, col = 7, lambda c: [PA, c]
    cons, _ = _programs([col(i % W) + col((3 * i + 1) % W) + [MUL] + col((5 * i + 2) % W) + [SUB] for i in range(66)], [])
    return W, cons, None


AIRS = {"hand": hand_made_air, "column": column_air, "wide": wide_air}


def group_starts(it):
    return [int(s) for s in sm.group_starts(*it)]


def multiplicity_columns(it):
    """per interaction the columns its multiplicity program reads"""
    inter, ispans, ibc = it
    out = []
    for _, _, s0 in inter.tolist():
        off, ln = ispans[s0].tolist()
        code, cols, i = ibc[off:off + ln].tolist(), [], 0
        while i < len(code):
            if code[i] in (PA, PC):
                cols += [code[i + 1]] if code[i] == PA else []
                i += 2
            else:
                i += 1
        out.append(cols)
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def cells(family, rng, w, n):
    """(w, n) canonical words"""
    if family == "random":
        return rng.integers(0, P, (w, n), dtype=np.uint32)
    if family == "edge":
        return ev.EDGE[rng.integers(0, len(ev.EDGE), (w, n))].astype(np.uint32)
    t = np.full((w, n), PM1, np.uint32)  # bound: every device word p - 1 ...
    t[:, 1::2] = 0                       # ... and every second lane all zero, so that neighbouring lanes differ
    return t


def ext_table(family, rng, n):
    """(n, 4) canonical coordinates: blpow / apow of the random and edge families"""
    return cells("edge" if family == "edge" else "random", rng, n, 4)


def bound_blpow(family, rng, n):
    """every coordinate of blpow[1..] at a centred extreme; blpow[0] (which no kernel reads) random"""
    sign = {"bound_pos": [1] * n, "bound_neg": [-1] * n, "bound_alt": [1 if j % 2 else -1 for j in range(n)]}[family]
    t = np.array([[WORD_HI if s > 0 else WORD_LO] * 4 for s in sign], np.uint32)
    t[0] = rng.integers(0, P, 4)
    return t


def bound_alpha(family):
    """the first product a_0 * centred(blpow[1]) has blpow[1]'s sign (a cell's word is non-negative): alpha's coordinates at the same
    extreme, so that seed and products pile up (coordinate 0 carries the bus id as well and lands elsewhere)"""
    return (WORD_LO,) * 4 if family == "bound_neg" else (WORD_HI,) * 4


def perm_inputs(name, family, rng, W, it, log_h):
    """(T, alpha, blpow) of one permutation-trace case, with planted rows: all multiplicity columns zero (no inversion on the row) and,
    on the column AIR, only ONE group active (its batch partners inactive)"""
    H = 1 << log_h
    T = cells(family, rng, W, H)
    n_bl = int(it[0][:, 1].max()) + 2
    mcols, starts = multiplicity_columns(it), group_starts(it)
    G = len(starts) - 1
    all_m = sorted({c for cs in mcols for c in cs})
    for r in range(H):
        if r % 7 == 3:
            T[all_m, r] = 0
        elif r % 7 == 5 and name == "column":
            keep = (r // 7) % G
            T[sorted({c for i, cs in enumerate(mcols) for c in cs if not starts[keep] <= i < starts[keep + 1]}), r] = 0
    if family.startswith("bound"):
        return T, bound_alpha(family), bound_blpow(family, rng, n_bl)
    return T, tuple(int(x) for x in ext_table(family, rng, 1)[0]), ext_table(family, rng, n_bl)


def vanishing_inputs(name, rng, W, it, log_h):
    """(T, alpha, blpow, interaction, rows): random non-zero cells; the chosen rows all carry row 0's cells, and alpha is minus the rest
    of ONE interaction's denominator there, so that exactly this denominator vanishes on exactly these rows — where every multiplicity
    of its group is non-zero (hand: interaction 4 of the five-member group, multiplicity col 3 * col 4, next to the constant
    multiplicities; column: interaction 4, the second member of a pair)"""
    H = 1 << log_h
    rows = sorted({min(r, H - 1) for r in VANISH_ROWS})
    T = rng.integers(1, P, (W, H), dtype=np.uint32)
    T[:, rows] = T[:, :1]
    blpow = ext_table("random", rng, int(it[0][:, 1].max()) + 2)
    i = 4
    _, ds = ref.interaction_values(T[:, :1], it, ref.ZERO, blpow)
    alpha = ref.ext_sub(ref.ZERO, tuple(int(x) for x in ds[i][0]))
    return T, alpha, blpow, i, rows


def quotient_inputs(family, rng, W, it, nc, log_n):
    """(lde, plde, apow, blpow) of one quotient case; plde = 4 G group columns, 4 phi columns and, as the specialised route reads them,
    4 columns that hold the sum of the group columns"""
    N = 1 << log_n
    bound = family == "bound"
    lde = cells("bound_pos" if bound else family, rng, W, N)
    if it is None:
        return lde, None, np.full((nc, 4), PM1, np.uint32) if bound else ext_table(family, rng, nc), None
    G = len(group_starts(it)) - 1
    plde = np.zeros((4 * G + 8, N), np.uint32)
    plde[:4 * G + 4] = cells("edge" if bound else family, rng, 4 * G + 4, N)
    plde[4 * G + 4:] = plde[:4 * G].reshape(G, 4, N).astype(np.uint64).sum(axis=0) % P
    n_bl = int(it[0][:, 1].max()) + 2
    M = nc + G + 3
    if bound:
        return lde, plde, np.full((M, 4), PM1, np.uint32), bound_blpow("bound_pos", rng, n_bl)
    return lde, plde, ext_table(family, rng, M), ext_table(family, rng, n_bl)


def perm_columns(q, phi, rowsum=None):
    """the reference's (G, n, 4), (n, 4) [, (n, 4)] as the columns the kernels write"""
    G, n = q.shape[0], q.shape[1]
    return np.concatenate([q.transpose(0, 2, 1).reshape(4 * G, n), phi.T] + ([rowsum.T] if rowsum is not None else []))


# ---- provers -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def provers(gpu):
    """get(air, kind) -> (Prover, W, cons, it): made once per module, the environment set while a prover is created and specialised"""
    torch, abi, prover = gpu
    made = {}

    def get(name, kind):
        if (name, kind) not in made:
            W, cons, it = AIRS[name]()
            with pytest.MonkeyPatch.context() as mp:
                for k in _ENV:
                    mp.delenv(k, raising=False)
                for k, v in PROVERS[kind].items():
                    mp.setenv(k, v)
                pr = prover.Prover(W, cons[0], cons[1], num_queries=4, pow_bits=0, interactions=it)
                if kind.startswith("jit"):
                    assert pr.specialise(), pr.specialised()
            info = pr.specialised()
            if kind == "jit-small":
                assert info["chunks"] >= 3 and len(pr.quotient_units()) >= 2, info
            if not kind.startswith("jit"):
                assert info["state"] != 1 and pr.quotient_units() == []
            if kind == "postfix" and it is not None:
                assert pr.logup_path() == 1
            if it is not None:
                assert (prover.logup_group_starts(it) == group_starts(it)).all()
            made[(name, kind)] = (pr, W, cons, it)
        return made[(name, kind)]

    yield get
    torch.cuda.synchronize()
    for pr, *_ in made.values():
        pr.close()


# ---- the permutation trace ---------------------------------------------------------------------------------------------------------
def run_perm(gpu, pr, it, T, log_h, alpha, blpow):
    """-> (columns (4 G + 4 or 8, H), rowsum (H, 4), the words behind both outputs still hold the sentinel)"""
    torch, abi, prover = gpu
    H, G = 1 << log_h, len(group_starts(it)) - 1
    n_cols = 4 * G + (8 if pr.specialised()["state"] == 1 else 4)
    d_t, d_bl, a = to_dev(torch, T), to_dev(torch, blpow), h4(alpha)
    d_perm, d_rs = sentinel(torch, (4 * G + 9) * H), sentinel(torch, 4 * H + 4)
    abi.check(prover.lib.pw_stage_logup_perm(pr._h, d_t.data_ptr(), log_h, a.ctypes.data, d_bl.data_ptr(), d_perm.data_ptr(), d_rs.data_ptr()),
              "pw_stage_logup_perm")
    perm, clean = split(torch, d_perm, n_cols * H)
    rs, clean_rs = split(torch, d_rs, 4 * H)
    return perm.reshape(n_cols, H), rs.reshape(H, 4), clean and clean_rs


def first_difference(got, want):
    """(column, row) of the first differing word, for the assertion message"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return None if not len(bad) else tuple(int(x) for x in bad[0])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PROVERS))
@pytest.mark.parametrize("name", ["hand", "column"])
def test_logup_perm(gpu, provers, name, kind):
    """logup_perm_kernel<FAST> / pwj_perm_* + rowsum_combine_kernel + the scan: one lane pair, the 256-lane block edge, two blocks (and,
    random on `forms` and `jit`, two 4096-row scan chunks); the group columns, d_rowsum, phi and — specialised — the row-sum columns"""
    pr, W, cons, it = provers(name, kind)
    starts = group_starts(it)
    jit = kind.startswith("jit")
    for log_h in (1, 2, 8, 9, 13):
        for family in PERM_FAMILIES[name]:
            if log_h == 13 and not (family == "random" and kind in ("forms", "jit")):
                continue
            rng = np.random.default_rng([1, log_h, PERM_FAMILIES["column"].index(family)])
            T, alpha, blpow = perm_inputs(name, family, rng, W, it, log_h)
            q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow)
            got, got_rs, clean = run_perm(gpu, pr, it, T, log_h, alpha, blpow)
            want = perm_columns(q, phi, rowsum if jit else None)
            assert clean, (log_h, family)
            assert (got == want).all(), (log_h, family, "column, row", first_difference(got, want))
            assert (got_rs == rowsum).all(), (log_h, family, "row, coordinate", first_difference(got_rs, rowsum))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["hand", "column"])
def test_vanishing_denominator(gpu, provers, name):
    """One interaction's denominator is exactly 0 on row 0, lanes 255 and 256 and the last row: its group's ONE inversion is of 0, whose
    inverse is 0 in every path (bb::inv, ext_inv_finish, batch_inverse's replacement of a zero norm, which must leave the batch
    partners' inverses alone): q_g = 0 for that group there, every other group and row as the reference has it, all four provers alike.
    On those rows EVERY member of the group has a non-zero multiplicity. A zero denominator under a zero multiplicity is NOT planted:
    there the interpreter skips the member and the specialised code multiplies it in, so q_g is the other members' sum on one path and
    0 on the other — both are right about 0 / 0, and no proof with such a row verifies anyway."""
    for log_h in (1, 9):
        _, W, cons, it = provers(name, "forms")
        starts = group_starts(it)
        T, alpha, blpow, i, rows = vanishing_inputs(name, np.random.default_rng([2, log_h]), W, it, log_h)
        q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow, vanishing=[(i, r) for r in rows])
        g = [k for k in range(len(starts) - 1) if starts[k] <= i < starts[k + 1]][0]
        ms, _ = ref.interaction_values(T, it, alpha, blpow)
        assert all(int(ms[m][r]) for m in range(starts[g], starts[g + 1]) for r in rows)
        assert not q[g][rows].any() and q[g][[r for r in range(1 << log_h) if r not in rows]].any(axis=1).all()
        for kind in PROVERS:
            pr = provers(name, kind)[0]
            got, got_rs, clean = run_perm(gpu, pr, it, T, log_h, alpha, blpow)
            want = perm_columns(q, phi, rowsum if kind.startswith("jit") else None)
            assert clean and (got == want).all() and (got_rs == rowsum).all(), (kind, log_h, first_difference(got, want))


# ---- the quotient ------------------------------------------------------------------------------------------------------------------
def run_quotient(gpu, pr, it, lde, plde, log_n, apow, alpha, blpow, S):
    torch, abi, prover = gpu
    N = 1 << log_n
    d_l, d_a, d_q = to_dev(torch, lde), to_dev(torch, apow), sentinel(torch, 4 * N + 4)
    n = C.c_uint32(0)
    if it is None:
        rc = prover.lib.pw_stage_quotient(pr._h, d_l.data_ptr(), None, log_n, d_a.data_ptr(), None, None, None, d_q.data_ptr(), C.byref(n))
    else:
        d_p, d_b, a, s = to_dev(torch, plde), to_dev(torch, blpow), h4(alpha), h4(S)
        rc = prover.lib.pw_stage_quotient(pr._h, d_l.data_ptr(), d_p.data_ptr(), log_n, d_a.data_ptr(), a.ctypes.data, d_b.data_ptr(), s.ctypes.data,
                                          d_q.data_ptr(), C.byref(n))
    abi.check(rc, "pw_stage_quotient")
    got, clean = split(torch, d_q, 4 * N)
    return got.reshape(4, N), clean, n.value


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PROVERS))
@pytest.mark.parametrize("name", list(AIRS))
def test_quotient(gpu, provers, name, kind):
    """quotient_logup_kernel / quotient_kernel + quotient_combine_kernel / pwj_quotient_* + quotient_logup_tail_kernel: the constraint
    and group sums, the boundary terms at rows j and (j + 2) mod N (the wrap rows N - 2 and N - 1 included), is_first / is_last /
    is_transition, Z_H's even / odd values; S and the bus challenge at their edges"""
    pr, W, cons, it = provers(name, kind)
    starts = group_starts(it) if it is not None else None
    nc = len(cons[1])
    for log_n in (1, 2, 8, 9):
        for f, family in enumerate(("random", "edge", "bound")):
            rng = np.random.default_rng([3, log_n, f])
            lde, plde, apow, blpow = quotient_inputs(family, rng, W, it, nc, log_n)
            if it is None:
                got, clean, n_chunks = run_quotient(gpu, pr, None, lde, None, log_n, apow, None, None, None)
                want = ref.quotient(lde, None, log_n, cons, None, None, apow).T
                assert clean and (got == want).all(), (log_n, family, first_difference(got, want))
                assert n_chunks > 1 or kind.startswith("jit"), n_chunks  # the interpreter splits 66 constraints at these heights
                continue
            sums = [ZERO4, ALL_PM1, rand_ext(rng)]
            for k, alpha in enumerate(scalar_set(rng)):
                S = sums[k % 3]
                got, clean, _ = run_quotient(gpu, pr, it, lde, plde, log_n, apow, alpha, blpow, S)
                want = ref.quotient(lde, plde, log_n, cons, it, starts, apow, alpha, blpow, S).T
                assert clean and (got == want).all(), (log_n, family, alpha, S, "coordinate, row", first_difference(got, want))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PROVERS))
def test_quotient_of_a_real_permutation_matrix(gpu, provers, kind):
    """the hand-made AIR with what a proof would hold: pw_stage_logup_perm's output (with the row sums as four more columns, as the
    specialised route keeps them) extended by pw_lde_batch, true powers of the challenges, S = phi(last row)"""
    torch, abi, prover = gpu
    pr, W, cons, it = provers("hand", kind)
    starts = group_starts(it)
    G, nc = len(starts) - 1, len(cons[1])
    for log_h in (4, 7, 8):
        rng = np.random.default_rng([4, log_h])
        H, N, log_n = 1 << log_h, 2 << log_h, log_h + 1
        T, alpha, _ = perm_inputs("hand", "random", rng, W, it, log_h)
        blpow = ref.ext_powers(rand_ext(rng), int(it[0][:, 1].max()) + 2).astype(np.uint32)
        apow = ref.ext_powers(rand_ext(rng), nc + G + 3, reversed_=True).astype(np.uint32)
        got, got_rs, _ = run_perm(gpu, pr, it, T, log_h, alpha, blpow)
        q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow)
        perm = perm_columns(q, phi, rowsum).astype(np.uint32)
        assert (got == perm[:len(got)]).all() and (got_rs == rowsum).all()
        mine = np.concatenate([got[:4 * G + 4], got_rs.T]).astype(np.uint32)  # (the interpreter routes leave the row sums in d_rowsum)
        d_m, d_c, d_p = to_dev(torch, mine), sentinel(torch, (4 * G + 8) * H), sentinel(torch, (4 * G + 8) * N)
        abi.check(prover.lib.pw_lde_batch(d_m.data_ptr(), 4 * G + 8, log_h, d_c.data_ptr(), d_p.data_ptr()), "pw_lde_batch")
        plde = om.from_monty(raw(torch, d_p)).reshape(4 * G + 8, N)
        assert (plde == sm.lde(perm.reshape(-1), 4 * G + 8, log_h).reshape(4 * G + 8, N)).all()
        lde = sm.lde(T.reshape(-1), W, log_h).reshape(W, N)
        S = tuple(int(x) for x in phi[H - 1])
        out, clean, _ = run_quotient(gpu, pr, it, lde, plde, log_n, apow, alpha, blpow, S)
        want = ref.quotient(lde, plde, log_n, cons, it, starts, apow, alpha, blpow, S).T
        assert clean and (out == want).all(), (log_h, first_difference(out, want))


# ---- the current-row sums ----------------------------------------------------------------------------------------------------------
def run_sums(gpu, pr, it, T, Pm, rows, apow, alpha, blpow, unit=-1, d_pm=None):
    """-> (parts (n_parts, 4, rows) as canonical values with the sentinel kept where a word still holds it, n_parts, clean)"""
    torch, abi, prover = gpu
    cap = max(pr.specialised()["chunks"], 1) + 1
    d_t, d_a, d_part = to_dev(torch, T), to_dev(torch, apow), sentinel(torch, cap * 4 * rows)
    n = C.c_uint32(0)
    if it is None:
        rc = prover.lib.pw_stage_quotient_sums(pr._h, d_t.data_ptr(), None, rows, 9, d_a.data_ptr(), None, None, unit, d_part.data_ptr(), C.byref(n))
    else:
        d_p = to_dev(torch, Pm) if d_pm is None else d_pm
        d_b, a = to_dev(torch, blpow), h4(alpha)
        ptr = d_p.data_ptr() + (0 if d_pm is None else 4 * rows * 4)  # a panel: behind its four guard columns
        rc = prover.lib.pw_stage_quotient_sums(pr._h, d_t.data_ptr(), ptr, rows, 9, d_a.data_ptr(), a.ctypes.data, d_b.data_ptr(), unit, d_part.data_ptr(),
                                               C.byref(n))
    abi.check(rc, "pw_stage_quotient_sums")
    words = raw(torch, d_part)
    n_parts = n.value
    assert 1 <= n_parts < cap
    parts = np.where(words == SENT, np.uint64(SENT), om.from_monty(np.where(words == SENT, 0, words).astype(np.uint32)).astype(np.uint64))
    return parts[:n_parts * 4 * rows].reshape(n_parts, 4, rows), n_parts, bool((words[n_parts * 4 * rows:] == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(PROVERS))
@pytest.mark.parametrize("name", list(AIRS))
def test_quotient_sums(gpu, provers, name, kind):
    """what the streamed route launches per sub-coset: quotient_logup_kernel<main_only>, quotient_kernel with Z^-1 = 1, the specialised
    chunk kernels — the parts' sum is the unscaled current-row value. On `jit-small` also every unit ALONE over a panel that holds only
    its own permutation columns between sentinel columns: a unit writes the parts of its chunks and no other, and the units' parts
    add up to the same value."""
    torch, abi, prover = gpu
    pr, W, cons, it = provers(name, kind)
    starts = group_starts(it) if it is not None else None
    G, nc = (len(starts) - 1 if it is not None else 0), len(cons[1])
    for rows in (2, 256, 512):
        for f, family in enumerate(("random", "edge", "bound")):
            rng = np.random.default_rng([5, rows, f])
            T, plde, apow, blpow = quotient_inputs(family, rng, W, it, nc, rows.bit_length() - 1)
            Pm = plde[:4 * G] if it is not None else None
            alpha = bound_alpha("bound_pos") if family == "bound" else rand_ext(rng)
            want = ref.quotient_sums(T, Pm, cons, it, starts, apow, alpha, blpow).T
            parts, n_parts, clean = run_sums(gpu, pr, it, T, Pm, rows, apow, alpha, blpow)
            assert clean and not (parts == SENT).any(), (rows, family)
            got = parts.sum(axis=0) % P
            assert (got == want).all(), (rows, family, "coordinate, row", first_difference(got, want))
            if kind != "jit-small":
                assert n_parts == 1 or kind == "jit"
                continue
            total, owned = np.zeros((4, rows), np.uint64), np.zeros(n_parts, int)
            for u, (g0, g1) in enumerate(pr.quotient_units()):
                d_panel = None
                if it is not None:
                    panel = np.full((4 * (g1 - g0) + 8, rows), SENT, np.uint32)
                    panel[4:4 + 4 * (g1 - g0)] = om.to_monty(np.ascontiguousarray(Pm[4 * g0:4 * g1]).reshape(-1)).reshape(-1, rows)
                    d_panel = raw_dev(torch, panel)
                parts, n_u, clean = run_sums(gpu, pr, it, T, None, rows, apow, alpha, blpow, unit=u, d_pm=d_panel)
                mine = [c for c in range(n_u) if not (parts[c] == SENT).any()]
                assert clean and n_u == n_parts and mine and all((parts[c] == SENT).all() for c in range(n_u) if c not in mine), (rows, family, u)
                owned[mine] += 1
                total = (total + parts[mine].sum(axis=0)) % P
            assert (owned == 1).all() and (total == want).all(), (rows, family, owned, first_difference(total, want))


# ---- the tail and the row-sum combination ------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_chunks", [1, 3, 64])
def test_logup_tail_and_rowsum_combine(gpu, n_chunks):
    """quotient_logup_tail_kernel and rowsum_combine_kernel take no program: parts of words p - 1 (64 of them leave 32 bits) and random
    ones; one lane pair, two lane pairs, two blocks; in place (d_q = d_part with one chunk, as the streamed route calls it) and not"""
    torch, abi, prover = gpu
    lib = prover.lib
    rng = np.random.default_rng(600 + n_chunks)
    for log_n in (1, 2, 9):
        N = 1 << log_n
        for kind in ("p-1", "random"):
            words = np.full((n_chunks, 4, N), P - 1, np.uint32) if kind == "p-1" else rng.integers(0, P, (n_chunks, 4, N), dtype=np.uint32)
            part = om.from_monty(words.reshape(-1)).reshape(n_chunks, 4, N)
            want_rs = ref.rowsum_combine(part)
            d_part = raw_dev(torch, words)
            d_rs, d_c4 = sentinel(torch, 4 * N + 4), sentinel(torch, 4 * N + 4)
            abi.check(lib.pw_stage_rowsum_combine(d_part.data_ptr(), n_chunks, N, d_rs.data_ptr(), d_c4.data_ptr()), "pw_stage_rowsum_combine")
            rs, clean = split(torch, d_rs, 4 * N)
            c4, clean4 = split(torch, d_c4, 4 * N)
            assert clean and clean4 and (rs.reshape(N, 4) == want_rs).all() and (c4.reshape(4, N) == want_rs.T).all(), (log_n, kind)
            family = "edge" if kind == "p-1" else "random"
            phi, sumq, tail = cells(family, rng, 4, N), cells(family, rng, 4, N), ext_table(family, rng, 3)
            d_phi, d_sq, d_t = to_dev(torch, phi), to_dev(torch, sumq), to_dev(torch, tail)
            for S in (ZERO4, ALL_PM1, rand_ext(rng)):
                want = ref.logup_tail(part, phi, sumq, log_n, tail, S).T
                s = h4(S)
                for in_place in ([False, True] if n_chunks == 1 else [False]):
                    buf = np.full(4 * N + 4, SENT, np.uint32)
                    buf[:4 * N] = words.reshape(-1)[:4 * N]
                    d_q = raw_dev(torch, buf) if in_place else sentinel(torch, 4 * N + 4)
                    src = d_q if in_place else d_part
                    abi.check(lib.pw_stage_logup_tail(src.data_ptr(), n_chunks, d_phi.data_ptr(), d_sq.data_ptr(), log_n, d_t.data_ptr(), s.ctypes.data,
                                                      d_q.data_ptr()), "pw_stage_logup_tail")
                    got, clean = split(torch, d_q, 4 * N)
                    assert clean and (got.reshape(4, N) == want).all(), (log_n, kind, S, in_place, first_difference(got.reshape(4, N), want))


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_malformed_arguments_are_refused_before_any_launch(gpu, provers):
    """-1 for NULL pointers, a scalar word >= p, logs out of range, a LogUp call on a prover without interactions and the reverse, a
    unit that does not exist; the outputs still hold their sentinel, and well-formed calls succeed afterwards"""
    torch, abi, prover = gpu
    lib = prover.lib
    lg, W, cons, it = provers("hand", "forms")
    jit = provers("hand", "jit-small")[0]
    plain = provers("wide", "forms")[0]
    rng = np.random.default_rng(700)
    d_m, d_o = to_dev(torch, rng.integers(0, P, 64 * 64, dtype=np.uint32)), sentinel(torch, 64 * 64)
    m, o = d_m.data_ptr(), d_o.data_ptr()
    e, big = h4((0, 1, 0, 0)), h4((0, 0, P, 0))
    s, bad = e.ctypes.data, big.ctypes.data
    n_units = len(jit.quotient_units())
    refused = [
        lib.pw_stage_logup_perm(None, m, 3, s, m, o, o), lib.pw_stage_logup_perm(lg._h, None, 3, s, m, o, o),
        lib.pw_stage_logup_perm(lg._h, m, 3, None, m, o, o), lib.pw_stage_logup_perm(lg._h, m, 3, bad, m, o, o),
        lib.pw_stage_logup_perm(lg._h, m, 3, s, None, o, o), lib.pw_stage_logup_perm(lg._h, m, 3, s, m, None, o),
        lib.pw_stage_logup_perm(lg._h, m, 3, s, m, o, None), lib.pw_stage_logup_perm(lg._h, m, 27, s, m, o, o),
        lib.pw_stage_logup_perm(plain._h, m, 3, s, m, o, o),
        lib.pw_stage_quotient(None, m, m, 3, m, s, m, s, o, None), lib.pw_stage_quotient(lg._h, None, m, 3, m, s, m, s, o, None),
        lib.pw_stage_quotient(lg._h, m, None, 3, m, s, m, s, o, None), lib.pw_stage_quotient(lg._h, m, m, 0, m, s, m, s, o, None),
        lib.pw_stage_quotient(lg._h, m, m, 28, m, s, m, s, o, None), lib.pw_stage_quotient(lg._h, m, m, 3, None, s, m, s, o, None),
        lib.pw_stage_quotient(lg._h, m, m, 3, m, bad, m, s, o, None), lib.pw_stage_quotient(lg._h, m, m, 3, m, s, None, s, o, None),
        lib.pw_stage_quotient(lg._h, m, m, 3, m, s, m, bad, o, None), lib.pw_stage_quotient(lg._h, m, m, 3, m, s, m, None, o, None),
        lib.pw_stage_quotient(lg._h, m, m, 3, m, s, m, s, None, None), lib.pw_stage_quotient(plain._h, m, m, 3, m, s, m, s, o, None),
        lib.pw_stage_quotient(plain._h, m, None, 3, m, s, None, None, o, None), lib.pw_stage_quotient(lg._h, m, None, 3, m, None, None, None, o, None),
        lib.pw_stage_quotient_sums(lg._h, m, m, 8, 0, m, s, m, -1, o, None), lib.pw_stage_quotient_sums(lg._h, m, m, 8, 28, m, s, m, -1, o, None),
        lib.pw_stage_quotient_sums(lg._h, m, m, 0, 4, m, s, m, -1, o, None), lib.pw_stage_quotient_sums(lg._h, None, m, 8, 4, m, s, m, -1, o, None),
        lib.pw_stage_quotient_sums(lg._h, m, None, 8, 4, m, s, m, -1, o, None), lib.pw_stage_quotient_sums(lg._h, m, m, 8, 4, m, bad, m, -1, o, None),
        lib.pw_stage_quotient_sums(lg._h, m, m, 8, 4, m, s, m, -1, None, None), lib.pw_stage_quotient_sums(lg._h, m, m, 8, 4, m, s, m, 0, o, None),
        lib.pw_stage_quotient_sums(jit._h, m, m, 8, 4, m, s, m, n_units, o, None), lib.pw_stage_quotient_sums(plain._h, m, m, 8, 4, m, s, m, -1, o, None),
        lib.pw_stage_logup_tail(None, 1, m, m, 3, m, s, o), lib.pw_stage_logup_tail(m, 0, m, m, 3, m, s, o), lib.pw_stage_logup_tail(m, 1, None, m, 3, m, s, o),
        lib.pw_stage_logup_tail(m, 1, m, None, 3, m, s, o), lib.pw_stage_logup_tail(m, 1, m, m, 0, m, s, o), lib.pw_stage_logup_tail(m, 1, m, m, 28, m, s, o),
        lib.pw_stage_logup_tail(m, 1, m, m, 3, None, s, o), lib.pw_stage_logup_tail(m, 1, m, m, 3, m, bad, o), lib.pw_stage_logup_tail(m, 1, m, m, 3, m, s, None),
        lib.pw_stage_rowsum_combine(None, 1, 8, o, o), lib.pw_stage_rowsum_combine(m, 0, 8, o, o), lib.pw_stage_rowsum_combine(m, 1, 0, o, o),
        lib.pw_stage_rowsum_combine(m, 1, 8, None, o), lib.pw_stage_rowsum_combine(m, 1, 8, o, None),
    ]
    assert refused == [-1] * len(refused), refused
    g0, g1 = C.c_uint32(), C.c_uint32()
    assert lib.pw_prover_quotient_unit_groups(jit._h, n_units, C.byref(g0), C.byref(g1)) == -1
    assert lib.pw_prover_quotient_unit_groups(lg._h, 0, C.byref(g0), C.byref(g1)) == -1 and lib.pw_prover_quotient_units(None) == 0
    assert (raw(torch, d_o) == SENT).all()
    abi.check(lib.pw_stage_rowsum_combine(m, 1, 8, o, o + 4 * 40), "pw_stage_rowsum_combine")
    abi.check(lib.pw_stage_logup_tail(m, 1, m, m, 3, m, s, o + 4 * 80), "pw_stage_logup_tail")
    r = raw(torch, d_o)
    assert not (r[:32] == SENT).any() and (r[32:40] == SENT).all() and not (r[40:72] == SENT).any() and not (r[80:112] == SENT).any()
    assert (r[112:] == SENT).all()
