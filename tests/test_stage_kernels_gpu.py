"""The kernels between the commitments and the proof words, one by one through their pw_stage_ entry points (include/powdr_prover.h),
against tests/_stage_ref.py (which tests/test_stage_ref_cpu.py ties to the oracle's field and to polynomial identities): the opening
weights and ext_dot_partial_kernel, ext_powers_kernel, deep_kernel, deep_logup_kernel<TWO>, ext_lincomb_kernel,
deep_from_combo_kernel, fri_fold_kernel, the LogUp prefix scan, quotient_split_kernel, row_layout_kernel, part_scatter_kernel and
ext_axpy_kernel. Field arithmetic is exact: every comparison is equality of every output word, and the words behind an output must
still hold the sentinel it started with.

Three input families. `random`: canonical words. `edge`: cells and table coordinates drawn from tests/_edge_values.EDGE (0, 1, p - 1,
the neighbours of p / 2, as canonical values and as device words). `bound_*`: every cell's device word and every coordinate of the
weight / gamma table at the centred extremes +-(p - 1) / 2 — a table no transcript produces — so that each multiply-add of
bb::ExtCentredAcc is a product of two operands AT their bound, four of them between two folds: all products positive, all negative,
signs alternating along the summed index (the table's), signs alternating across lanes."""
import numpy as np
import pytest

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _edge_values as ev
from tests import _stage_ref as ref
from tests.test_prover_gpu import gpu  # noqa: F401  (the module-level fixture: torch, abi, prover — or a skip without a GPU)

P = om.P
HALF = (P - 1) // 2
SENT = 0x7FFFFFFF  # above p - 1 and above (p - 1) / 2: neither a field word nor a centred coordinate
INVALID = 1        # hipErrorInvalidValue
ZERO4, ONE4, ALL_PM1, X4 = (0, 0, 0, 0), (1, 0, 0, 0), (P - 1,) * 4, (0, 1, 0, 0)
FAMILIES = ["random", "edge", "bound_pos", "bound_neg", "bound_alt_table", "bound_alt_lane"]
BOUND = FAMILIES[2:]
WORD_HI, WORD_LO = ev.word(HALF), ev.word(HALF + 1)  # the canonical values whose device words centre to +(p-1)/2 and -(p-1)/2
WA, WB = (1, 3, 4, 5, 7, 8, 9), (1, 3, 4, 7, 8)      # every residue mod 4 of both column loops of deep_kernel / ext_lincomb_kernel


# ---- inputs ------------------------------------------------------------------------------------------------------------------------
def make_cells(family, rng, w, n, lane_axis=1):
    """(w, n) canonical words; the summed (table) index is the other axis than lane_axis"""
    if family == "random":
        return rng.integers(0, P, (w, n), dtype=np.uint32)
    if family == "edge":
        return ev.EDGE[rng.integers(0, len(ev.EDGE), (w, n))]
    hi = np.ones((w, n), bool)
    if family == "bound_alt_lane":
        hi[(slice(None), slice(1, None, 2)) if lane_axis == 1 else (slice(1, None, 2), slice(None))] = False
    return np.where(hi, WORD_HI, WORD_LO).astype(np.uint32)


def make_table(family, rng, n):
    """(n, 4) int32: centred representatives of Montgomery words, the form the kernels read"""
    if family == "random":
        return ref.centred_encode(rng.integers(0, P, (n, 4), dtype=np.uint32))
    if family == "edge":
        return ref.centred_encode(ev.EDGE[rng.integers(0, len(ev.EDGE), (n, 4))])
    sign = np.ones(n, np.int32)
    if family == "bound_neg":
        sign[:] = -1
    elif family == "bound_alt_table":
        sign[1::2] = -1
    return np.repeat((sign * HALF)[:, None], 4, axis=1).astype(np.int32)


def rand_ext(rng):
    return tuple(int(x) for x in rng.integers(0, P, 4))


def scalar_set(rng):
    """an extension scalar at its edges: random, 0, 1, all p - 1, X"""
    return [rand_ext(rng), ZERO4, ONE4, ALL_PM1, X4]


def points(rng):
    """opening points whose denominators x_j - zeta never vanish on the shifted domain: a non-zero higher coordinate, or the
    base-field 0 and 1 (31 w^j is neither: 31 generates the whole group, so it lies in no subgroup of 2-power order)"""
    return [rand_ext(rng), ZERO4, ONE4, rand_ext(rng), ALL_PM1, X4]


def h4(e):
    """a host extension scalar: 4 canonical words"""
    return np.array(e, dtype=np.uint32)


# ---- device plumbing ---------------------------------------------------------------------------------------------------------------
def to_dev(torch, canonical):
    return torch.from_numpy(om.to_monty(np.ascontiguousarray(canonical, dtype=np.uint32).reshape(-1)).view(np.int32)).cuda()


def raw_dev(torch, a):
    """words as they are (tables, index arrays, prepared buffers)"""
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int32).copy()).cuda()


def sentinel(torch, n_words):
    return torch.full((n_words,), SENT, dtype=torch.int32, device="cuda")


def raw(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def split(torch, t, n_words):
    """(the canonical values of the first n_words Montgomery words, whether everything behind them is still the sentinel)"""
    r = raw(torch, t)
    return om.from_monty(r[:n_words]), bool((r[n_words:] == SENT).all()) and len(r) > n_words


# ---- opening weights ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("on_coefficients", [0, 1])
def test_opening_weights(gpu, on_coefficients):
    """barycentric_weights_kernel / zeta_weights_kernel: one and two blocks, log_h = 0 of the coefficient kind, zeta at its edges
    (zeta = 1 lies IN the trace domain: zeta^H - 1 = 0 and every barycentric weight is 0); the stored words are the centred encoding"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(10 + on_coefficients)
    for log_h in ([0] if on_coefficients else []) + [1, 2, 8, 9]:
        H = 1 << log_h
        for zeta in scalar_set(rng):
            d_w = sentinel(torch, (H + 1) * 4)
            z = h4(zeta)
            abi.check(prover.lib.pw_stage_opening_weights(z.ctypes.data, log_h, on_coefficients, d_w.data_ptr()), "pw_stage_opening_weights")
            got = raw(torch, d_w).view(np.int32)
            want = (ref.coefficient_weights if on_coefficients else ref.barycentric_weights)(zeta, log_h)
            assert (got[4 * H:] == SENT).all(), (log_h, zeta)
            assert (got[:4 * H].reshape(H, 4) == ref.centred_encode(want)).all(), (log_h, zeta)


# ---- ext_dot -----------------------------------------------------------------------------------------------------------------------
def _ext_dot_case(torch, abi, prover, d_cols, stride, n_cols, length, d_w, d_w2, want, want2, tag):
    d_o, d_o2 = sentinel(torch, (n_cols + 1) * 4), sentinel(torch, (n_cols + 1) * 4)
    abi.check(prover.lib.pw_stage_ext_dot(d_cols.data_ptr(), stride, n_cols, length, d_w.data_ptr(), d_w2.data_ptr() if d_w2 is not None else None,
                                          d_o.data_ptr(), d_o2.data_ptr() if d_w2 is not None else None), "pw_stage_ext_dot")
    got, clean = split(torch, d_o, 4 * n_cols)
    assert clean and (got.reshape(n_cols, 4) == want[:n_cols]).all(), tag
    got2, clean2 = split(torch, d_o2, 4 * n_cols if d_w2 is not None else 0)
    assert clean2 and (d_w2 is None or (got2.reshape(n_cols, 4) == want2[:n_cols]).all()), tag


@pytest.mark.gpu
@pytest.mark.parametrize("length", [2, 64, 128, 8192, 16384])
def test_ext_dot(gpu, length):
    """ext_dot_partial_kernel<1> and <2> + ext_dot_final_kernel: the 64-column tile's edge and blockIdx.y > 0, one and two 64-row LDS
    tiles, one and two 8192-row chunks, a column stride past the length; the bound family at (65, 16384) and (64, 128)"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(20 + length)
    stride = length + (5 if length in (64, 16384) else 0)
    for family in ("random", "edge"):
        cells = make_cells(family, rng, 130, stride)
        d_cols = to_dev(torch, cells)
        t1, t2 = make_table(family, rng, length), make_table("random", rng, length)
        d_w, d_w2 = raw_dev(torch, t1), raw_dev(torch, t2)
        want, want2 = ref.ext_dot(cells[:, :length], ref.centred_decode(t1), ref.centred_decode(t2))
        for n_cols in (1, 63, 64, 65, 130):
            _ext_dot_case(torch, abi, prover, d_cols, stride, n_cols, length, d_w, None, want, None, (family, n_cols, 1))
            _ext_dot_case(torch, abi, prover, d_cols, stride, n_cols, length, d_w, d_w2, want, want2, (family, n_cols, 2))
    if length in (128, 16384):
        n_cols = 64 if length == 128 else 65
        for family in BOUND:
            cells = make_cells(family, rng, n_cols, length, lane_axis=0)
            d_cols = to_dev(torch, cells)
            t1 = make_table(family, rng, length)
            t2 = -t1  # the second vector's products carry the opposite signs
            d_w, d_w2 = raw_dev(torch, t1), raw_dev(torch, t2)
            want, want2 = ref.ext_dot(cells, ref.centred_decode(t1), ref.centred_decode(t2))
            _ext_dot_case(torch, abi, prover, d_cols, length, n_cols, length, d_w, None, want, None, (family, 1))
            _ext_dot_case(torch, abi, prover, d_cols, length, n_cols, length, d_w, d_w2, want, want2, (family, 2))


# ---- ext_powers --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_ext_powers(gpu):
    """ext_powers_kernel: around one block (255, 256, 257), several blocks, both orders, both output forms, the base at its edges"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(30)
    for base in scalar_set(rng):
        b = h4(base)
        full = ref.ext_powers(base, 1000)
        for n in (1, 2, 255, 256, 257, 1000):
            for reversed_ in (0, 1):
                want = full[:n][::-1] if reversed_ else full[:n]
                for centred in (0, 1):
                    d_o = sentinel(torch, (n + 1) * 4)
                    abi.check(prover.lib.pw_stage_ext_powers(b.ctypes.data, n, reversed_, centred, d_o.data_ptr()), "pw_stage_ext_powers")
                    r = raw(torch, d_o)
                    assert (r[4 * n:] == SENT).all(), (base, n, reversed_, centred)
                    if centred:
                        assert (r[:4 * n].view(np.int32).reshape(n, 4) == ref.centred_encode(want)).all(), (base, n, reversed_)
                    else:
                        assert (om.from_monty(r[:4 * n]).reshape(n, 4) == want).all(), (base, n, reversed_)
    d_o = sentinel(torch, 8)
    b = h4(X4)
    assert prover.lib.pw_stage_ext_powers(b.ctypes.data, (1 << 24) + 1, 0, 1, d_o.data_ptr()) == INVALID
    assert (raw(torch, d_o) == SENT).all()


# ---- DEEP --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [1, 2, 9])
def test_deep(gpu, log_n):
    """deep_kernel: every residue mod 4 of the wa loop and of the wb loop (whose leftover columns no proof reaches: the provers pass
    wb = 8), one lane pair to two blocks, the subtracted sum at 0 / all p - 1 / random, all families"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(40 + log_n)
    N = 1 << log_n
    zetas, sums = points(rng), [ZERO4, ALL_PM1, rand_ext(rng)]
    i = 0
    for family in FAMILIES:
        a, b = make_cells(family, rng, max(WA), N), make_cells(family, rng, max(WB), N)
        d_a, d_b = to_dev(torch, a), to_dev(torch, b)
        for wa in WA:
            for wb in WB:
                table = make_table(family, rng, wa + wb)
                d_g, g = raw_dev(torch, table), ref.centred_decode(table)
                for total in sums:
                    zeta = zetas[i % len(zetas)]
                    i += 1
                    s, z = h4(total), h4(zeta)
                    d_v = sentinel(torch, (N + 1) * 4)
                    abi.check(prover.lib.pw_stage_deep(d_a.data_ptr(), wa, d_b.data_ptr(), wb, log_n, d_g.data_ptr(), s.ctypes.data, z.ctypes.data,
                                                       d_v.data_ptr()), "pw_stage_deep")
                    got, clean = split(torch, d_v, 4 * N)
                    assert clean and (got.reshape(N, 4) == ref.deep(a[:wa], b[:wb], g, total, zeta, log_n)).all(), (family, wa, wb, total, zeta)


@pytest.mark.gpu
@pytest.mark.parametrize("two_point", [False, True], ids=["one_point", "two_point"])
@pytest.mark.parametrize("log_n", [1, 2, 9])
def test_deep_logup(gpu, log_n, two_point):
    """deep_logup_kernel<false> / <true>: the W loop's and the Wp loop's leftover columns (Wp = 4 (n_groups + 1) in every proof), Wp = 0
    of a constraints-only two-point AIR, gK at its edges, all families"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(50 + 2 * log_n + two_point)
    N = 1 << log_n
    pts, sums = points(rng), [ZERO4, ALL_PM1, rand_ext(rng), rand_ext(rng)]
    gks = [ZERO4, ONE4, rand_ext(rng), ALL_PM1] if two_point else [None]
    i = 0
    for family in FAMILIES:
        lde, plde, qlde = make_cells(family, rng, 9, N), make_cells(family, rng, 8, N), make_cells(family, rng, 8, N)
        d_l, d_p, d_q = to_dev(torch, lde), to_dev(torch, plde), to_dev(torch, qlde)
        for W in (1, 4, 6, 9):
            for Wp in ((0,) if two_point else ()) + (4, 5, 7, 8):
                table = make_table(family, rng, W + 2 * Wp + 8)
                d_g, g = raw_dev(torch, table), ref.centred_decode(table)
                for gK in gks:
                    i += 1
                    sum1, sum2 = sums[i % 4], sums[(i // 4 + 1) % 4]
                    zeta, gzeta = pts[i % len(pts)], pts[(i + 1 + i // len(pts)) % len(pts)]
                    s1, s2, z, gz = h4(sum1), h4(sum2), h4(zeta), h4(gzeta)
                    k = h4(gK) if gK is not None else None
                    d_v = sentinel(torch, (N + 1) * 4)
                    abi.check(prover.lib.pw_stage_deep_logup(d_l.data_ptr(), W, d_p.data_ptr() if Wp else None, Wp, d_q.data_ptr(), log_n,
                                                             d_g.data_ptr(), k.ctypes.data if k is not None else None, s1.ctypes.data,
                                                             s2.ctypes.data, z.ctypes.data, gz.ctypes.data, d_v.data_ptr()), "pw_stage_deep_logup")
                    got, clean = split(torch, d_v, 4 * N)
                    want = ref.deep_logup(lde[:W], plde[:Wp], qlde, g, sum1, sum2, zeta, gzeta, log_n, gK)
                    assert clean and (got.reshape(N, 4) == want).all(), (family, W, Wp, gK, sum1, sum2, zeta, gzeta)


@pytest.mark.gpu
@pytest.mark.parametrize("length", [2, 4, 512, 1024])
def test_ext_lincomb(gpu, length):
    """ext_lincomb_kernel (the resident route takes it from 2^16 rows on, the streamed one always): one lane to two blocks of lane
    pairs, every residue mod 4 of both loops, with and without the second combination, all families"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(60 + length)
    for family in FAMILIES:
        a, b = make_cells(family, rng, max(WA), length), make_cells(family, rng, max(WB), length)
        d_a, d_b = to_dev(torch, a), to_dev(torch, b)
        for wa in WA:
            for wb in WB:
                table = make_table(family, rng, wa + wb + 8 + wb)
                d_g, g = raw_dev(torch, table), ref.centred_decode(table)
                for second in (0, wa + wb + 8):
                    n_out = 8 if second else 4
                    d_o = sentinel(torch, 8 * length + 4)
                    abi.check(prover.lib.pw_stage_ext_lincomb(d_a.data_ptr(), wa, d_b.data_ptr(), wb, length, d_g.data_ptr(), second, d_o.data_ptr()),
                              "pw_stage_ext_lincomb")
                    got, clean = split(torch, d_o, n_out * length)
                    assert clean and (got.reshape(n_out, length) == ref.ext_lincomb(a[:wa], b[:wb], g, second)).all(), (family, wa, wb, second)


@pytest.mark.gpu
def test_ext_lincomb_refusals(gpu):
    """an odd length, and a matrix / output pointer that the 8-byte loads and stores cannot take: hipErrorInvalidValue, nothing written"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(61)
    d_a, d_b = to_dev(torch, make_cells("random", rng, 3, 8)), to_dev(torch, make_cells("random", rng, 3, 8))
    d_g = raw_dev(torch, make_table("random", rng, 16))
    d_o = sentinel(torch, 8 * 8 + 4)
    a, b, g, o = d_a.data_ptr(), d_b.data_ptr(), d_g.data_ptr(), d_o.data_ptr()
    lib = prover.lib
    assert lib.pw_stage_ext_lincomb(a, 2, b, 2, 3, g, 0, o) == INVALID
    assert lib.pw_stage_ext_lincomb(a + 4, 2, b, 2, 4, g, 0, o) == INVALID
    assert lib.pw_stage_ext_lincomb(a, 2, b + 4, 2, 4, g, 0, o) == INVALID
    assert lib.pw_stage_ext_lincomb(a, 2, b, 2, 4, g, 0, o + 4) == INVALID
    assert lib.pw_stage_ext_lincomb(a, 2, b, 2, 0, g, 0, o) == -1
    assert lib.pw_stage_ext_lincomb(a, 2, b, 2, 4, None, 0, o) == -1
    assert (raw(torch, d_o) == SENT).all()
    abi.check(lib.pw_stage_ext_lincomb(a, 2, b, 2, 4, g, 0, o), "pw_stage_ext_lincomb")
    assert not (raw(torch, d_o)[:16] == SENT).any()


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [1, 2, 9])
def test_deep_from_combo(gpu, log_n):
    """deep_from_combo_kernel: with and without the second term, the eight quotient columns and their gamma powers in all families"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(70 + log_n)
    N = 1 << log_n
    pts, sums = points(rng), [ZERO4, ALL_PM1, rand_ext(rng)]
    i = 0
    for family in FAMILIES:
        for rep in range(3):
            glde, qlde = make_cells(family, rng, 8, N), make_cells(family, rng, 8, N)
            table = make_table(family, rng, 8)
            d_gl, d_q, d_g, gq = to_dev(torch, glde), to_dev(torch, qlde), raw_dev(torch, table), ref.centred_decode(table)
            for two in (0, 1):
                i += 1
                sum1, sum2, zeta, gzeta = sums[i % 3], sums[(i + rep) % 3], pts[i % len(pts)], pts[(i + 2) % len(pts)]
                s1, s2, z, gz = h4(sum1), h4(sum2), h4(zeta), h4(gzeta)
                d_v = sentinel(torch, (N + 1) * 4)
                abi.check(prover.lib.pw_stage_deep_from_combo(d_gl.data_ptr(), d_q.data_ptr(), log_n, d_g.data_ptr(), s1.ctypes.data, s2.ctypes.data,
                                                              z.ctypes.data, gz.ctypes.data, two, d_v.data_ptr()), "pw_stage_deep_from_combo")
                got, clean = split(torch, d_v, 4 * N)
                want = ref.deep_from_combo(glde, qlde, gq, sum1, sum2, zeta, gzeta, bool(two), log_n)
                assert clean and (got.reshape(N, 4) == want).all(), (family, two, sum1, sum2, zeta, gzeta)


@pytest.mark.gpu
def test_gamma_table_of_the_prover_feeds_deep(gpu):
    """the centred table the provers build (ext_powers, centred) is the form the tests above feed by hand: powers of gamma from
    pw_stage_ext_powers, then pw_stage_deep over the LDE of a small trace and eight more columns = the reference with true powers"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(80)
    W, log_h = 5, 4
    H, N, log_n = 1 << log_h, 2 << log_h, log_h + 1
    t = rng.integers(0, P, W * H, dtype=np.uint32)
    q = rng.integers(0, P, (8, N), dtype=np.uint32)
    gamma, total, zeta = rand_ext(rng), rand_ext(rng), rand_ext(rng)
    d_t, d_q = to_dev(torch, t), to_dev(torch, q)
    d_c, d_l = sentinel(torch, W * H), sentinel(torch, W * N)
    abi.check(prover.lib.pw_lde_batch(d_t.data_ptr(), W, log_h, d_c.data_ptr(), d_l.data_ptr()), "pw_lde_batch")
    d_g, d_v = sentinel(torch, (W + 8 + 1) * 4), sentinel(torch, (N + 1) * 4)
    gm, s, z = h4(gamma), h4(total), h4(zeta)
    abi.check(prover.lib.pw_stage_ext_powers(gm.ctypes.data, W + 8, 0, 1, d_g.data_ptr()), "pw_stage_ext_powers")
    abi.check(prover.lib.pw_stage_deep(d_l.data_ptr(), W, d_q.data_ptr(), 8, log_n, d_g.data_ptr(), s.ctypes.data, z.ctypes.data, d_v.data_ptr()),
              "pw_stage_deep")
    got, clean = split(torch, d_v, 4 * N)
    lde = sm.lde(t, W, log_h).reshape(W, N)
    assert clean and (got.reshape(N, 4) == ref.deep(lde, q, ref.ext_powers(gamma, W + 8), total, zeta, log_n)).all()


# ---- FRI ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log_size", [1, 2, 9, 10])
def test_fri_fold(gpu, log_size):
    """fri_fold_kernel: one lane to two blocks, the first round's shift, a later round's and none, beta at its edges, rows with a = b
    (the odd part vanishes) and a = -b (the even part does)"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(90 + log_size)
    n = 1 << log_size
    half = n // 2
    v_random = rng.integers(0, P, (n, 4), dtype=np.uint32)
    v_edge = ev.EDGE[rng.integers(0, len(ev.EDGE), (n, 4))].astype(np.uint32)
    v_edge[half::3] = v_edge[:half:3]
    v_edge[half + 1::3] = (P - v_edge[1:half:3]) % P
    for name, v in (("random", v_random), ("edge", v_edge)):
        d_v = to_dev(torch, v)
        for shift in (ref.SHIFT, ref.SHIFT * ref.SHIFT, 1):
            for beta in (ZERO4, ONE4, ALL_PM1, rand_ext(rng)):
                b = h4(beta)
                d_o = sentinel(torch, (half + 1) * 4)
                abi.check(prover.lib.pw_stage_fri_fold(d_v.data_ptr(), log_size, shift, b.ctypes.data, d_o.data_ptr()), "pw_stage_fri_fold")
                got, clean = split(torch, d_o, 4 * half)
                assert clean and (got.reshape(half, 4) == ref.fri_fold(v, log_size, shift, beta)).all(), (name, shift, beta)


# ---- the LogUp prefix scan ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("H", [2, 256, 4096, 8192, 65536])
def test_logup_scan(gpu, H):
    """scan_block_totals_kernel, scan_totals_kernel, scan_write_kernel: one 4096-row block (partly filled, full), two, sixteen; zeros,
    all p - 1 (every addition wraps), one non-zero row at the end of the first block (it must reach every later block), random"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(H)
    one_hot = np.zeros((H, 4), np.uint32)
    one_hot[min(H, 4096) - 1] = rand_ext(rng)
    for name, rows in (("zeros", np.zeros((H, 4), np.uint32)), ("p-1", np.full((H, 4), P - 1, np.uint32)), ("one_hot", one_hot),
                       ("random", rng.integers(0, P, (H, 4), dtype=np.uint32))):
        d_in, d_o = to_dev(torch, rows), sentinel(torch, 4 * H + 1)
        abi.check(prover.lib.pw_stage_logup_scan(d_in.data_ptr(), H, d_o.data_ptr()), "pw_stage_logup_scan")
        got, clean = split(torch, d_o, 4 * H)
        assert clean and (got.reshape(4, H) == ref.scan(rows)).all(), name


# ---- the small kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("log_h", [0, 1, 8, 9])
def test_quotient_split(gpu, log_h):
    """quotient_split_kernel: the single-row special case, one lane pair, one and two blocks"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(110 + log_h)
    H = 1 << log_h
    for family in ("random", "edge"):
        cbr = make_cells(family, rng, 4, 2 * H)
        d_c, d_o = to_dev(torch, cbr), sentinel(torch, 8 * H + 1)
        abi.check(prover.lib.pw_stage_quotient_split(d_c.data_ptr(), log_h, d_o.data_ptr()), "pw_stage_quotient_split")
        got, clean = split(torch, d_o, 8 * H)
        assert clean and (got.reshape(8, H) == ref.quotient_split(cbr, log_h)).all(), family


@pytest.mark.gpu
@pytest.mark.parametrize("log_n", [1, 2, 9])
def test_row_layout(gpu, log_n):
    """row_layout_kernel on both domains: next-row columns with the trace's step and the LDE's, a column named twice, the three
    selectors; the matrix in front stays as it was and nothing is written behind the columns asked for"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(120 + log_n)
    n, w1, next_cols = 1 << log_n, 3, [2, 0, 2]
    d_next = raw_dev(torch, np.array(next_cols, np.uint32))
    for family in ("random", "edge"):
        m = make_cells(family, rng, w1, n)
        front = om.to_monty(m.reshape(-1))
        for trace_domain in (0, 1):
            for n_next in (0, 3):
                for step in (1, 2):
                    for selectors in (0, 1):
                        n_new = n_next + 3 * selectors
                        buf = np.full((w1 + n_new + 1) * n, SENT, np.uint32)
                        buf[:w1 * n] = front
                        d_m = raw_dev(torch, buf)
                        abi.check(prover.lib.pw_stage_row_layout(d_m.data_ptr(), log_n, w1, d_next.data_ptr() if n_next else None, n_next, step,
                                                                 selectors, trace_domain), "pw_stage_row_layout")
                        r = raw(torch, d_m)
                        tag = (family, trace_domain, n_next, step, selectors)
                        assert (r[:w1 * n] == front).all() and (r[(w1 + n_new) * n:] == SENT).all(), tag
                        want = ref.row_layout(m, log_n, next_cols[:n_next], step, bool(selectors), bool(trace_domain))
                        assert (om.from_monty(r[w1 * n:(w1 + n_new) * n]).reshape(n_new, n) == want).all(), tag


@pytest.mark.gpu
def test_part_scatter(gpu):
    """part_scatter_kernel: plain sums of words (all p - 1: 64 of them leave 32 bits), one row pair and two blocks, every sub-coset r of
    2 and of 4: a call writes the rows r + 2^b i and no other"""
    torch, abi, prover = gpu
    rng = np.random.default_rng(130)
    for n_chunks in (1, 3, 64):
        for m in (2, 300):
            for kind in ("p-1", "random"):
                part = np.full((n_chunks, 4, m), P - 1, np.uint32) if kind == "p-1" else rng.integers(0, P, (n_chunks, 4, m), dtype=np.uint32)
                d_p = raw_dev(torch, part)
                for b in (1, 2):
                    N = m << b
                    d_o = sentinel(torch, 4 * N + 1)
                    want = np.full((4, N), SENT, np.uint64)
                    for r in rng.permutation(1 << b).tolist():
                        abi.check(prover.lib.pw_stage_part_scatter(d_p.data_ptr(), n_chunks, m, b, r, N, d_o.data_ptr()), "pw_stage_part_scatter")
                        want = ref.part_scatter(part, b, r, want)
                        got = raw(torch, d_o)
                        assert got[4 * N] == SENT and (got[:4 * N].reshape(4, N) == want).all(), (n_chunks, m, kind, b, r)
                    assert not (want == SENT).any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 257])
def test_ext_axpy(gpu, n):
    torch, abi, prover = gpu
    rng = np.random.default_rng(140 + n)
    x, y = rng.integers(0, P, (n, 4), dtype=np.uint32), ev.EDGE[rng.integers(0, len(ev.EDGE), (n, 4))]
    d_x = to_dev(torch, x)
    for a in (None, ZERO4, rand_ext(rng), ALL_PM1):
        buf = np.full((n + 1) * 4, SENT, np.uint32)
        buf[:4 * n] = om.to_monty(y.reshape(-1))
        d_y = raw_dev(torch, buf)
        k = h4(a) if a is not None else None
        abi.check(prover.lib.pw_stage_ext_axpy(d_y.data_ptr(), k.ctypes.data if k is not None else None, d_x.data_ptr(), n), "pw_stage_ext_axpy")
        got, clean = split(torch, d_y, 4 * n)
        assert clean and (got.reshape(n, 4) == ref.ext_axpy(y, a, x)).all(), a


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_malformed_arguments_are_refused_before_any_launch(gpu):
    """-1 for NULL pointers, scalar words >= p, logs out of range and zero sizes; hipErrorInvalidValue for the alignments the wrappers
    check themselves; the output buffers still hold their sentinel afterwards, and a well-formed call still succeeds"""
    torch, abi, prover = gpu
    lib = prover.lib
    rng = np.random.default_rng(150)
    d_m = to_dev(torch, make_cells("random", rng, 8, 64))
    d_g = raw_dev(torch, make_table("random", rng, 64))
    d_o = sentinel(torch, 1024)
    m, g, o = d_m.data_ptr(), d_g.data_ptr(), d_o.data_ptr()
    e, big = h4(X4), h4((P, 0, 0, 0))
    s, bad = e.ctypes.data, big.ctypes.data
    refused = [
        lib.pw_stage_opening_weights(None, 3, 0, o), lib.pw_stage_opening_weights(bad, 3, 0, o), lib.pw_stage_opening_weights(s, 27, 1, o),
        lib.pw_stage_opening_weights(s, 3, 0, None),
        lib.pw_stage_ext_dot(None, 8, 2, 8, g, None, o, None), lib.pw_stage_ext_dot(m, 8, 0, 8, g, None, o, None),
        lib.pw_stage_ext_dot(m, 8, 2, 0, g, None, o, None), lib.pw_stage_ext_dot(m, 7, 2, 8, g, None, o, None),
        lib.pw_stage_ext_dot(m, 8, 2, 8, g, g, o, None), lib.pw_stage_ext_dot(m, 8, 2, 8, None, None, o, None),
        lib.pw_stage_ext_powers(None, 4, 0, 0, o), lib.pw_stage_ext_powers(bad, 4, 0, 0, o), lib.pw_stage_ext_powers(s, 4, 0, 0, None),
        lib.pw_stage_deep(m, 2, m, 2, 0, g, s, s, o), lib.pw_stage_deep(m, 2, m, 2, 28, g, s, s, o), lib.pw_stage_deep(None, 2, m, 2, 3, g, s, s, o),
        lib.pw_stage_deep(m, 2, m, 2, 3, g, None, s, o), lib.pw_stage_deep(m, 2, m, 2, 3, g, s, bad, o), lib.pw_stage_deep(m, 0, m, 0, 3, g, s, s, o),
        lib.pw_stage_deep_logup(m, 2, None, 4, m, 3, g, None, s, s, s, s, o), lib.pw_stage_deep_logup(m, 2, m, 4, None, 3, g, None, s, s, s, s, o),
        lib.pw_stage_deep_logup(m, 2, m, 4, m, 0, g, None, s, s, s, s, o), lib.pw_stage_deep_logup(m, 2, m, 4, m, 3, g, bad, s, s, s, s, o),
        lib.pw_stage_deep_from_combo(m, m, 0, g, s, s, s, s, 1, o), lib.pw_stage_deep_from_combo(m, None, 3, g, s, s, s, s, 1, o),
        lib.pw_stage_deep_from_combo(m, m, 3, g, s, s, s, None, 0, o),
        lib.pw_stage_fri_fold(m, 0, 31, s, o), lib.pw_stage_fri_fold(m, 28, 31, s, o), lib.pw_stage_fri_fold(m, 3, 0, s, o),
        lib.pw_stage_fri_fold(m, 3, P, s, o), lib.pw_stage_fri_fold(m, 3, 31, bad, o), lib.pw_stage_fri_fold(None, 3, 31, s, o),
        lib.pw_stage_logup_scan(m, 0, o), lib.pw_stage_logup_scan(None, 8, o), lib.pw_stage_logup_scan(m, 8, None),
        lib.pw_stage_quotient_split(m, 27, o), lib.pw_stage_quotient_split(None, 3, o),
        lib.pw_stage_row_layout(None, 3, 2, g, 1, 1, 1, 0), lib.pw_stage_row_layout(o, 0, 2, g, 1, 1, 1, 0), lib.pw_stage_row_layout(o, 3, 2, None, 1, 1, 1, 0),
        lib.pw_stage_part_scatter(m, 2, 8, 1, 2, 16, o), lib.pw_stage_part_scatter(m, 2, 8, 1, 0, 15, o), lib.pw_stage_part_scatter(m, 0, 8, 1, 0, 16, o),
        lib.pw_stage_part_scatter(m, 2, 0, 1, 0, 16, o), lib.pw_stage_part_scatter(None, 2, 8, 1, 0, 16, o),
        lib.pw_stage_ext_axpy(o, s, m, 0), lib.pw_stage_ext_axpy(o, bad, m, 4), lib.pw_stage_ext_axpy(None, s, m, 4),
    ]
    assert refused == [-1] * len(refused), refused
    assert lib.pw_stage_ext_dot(m, 8, 2, 8, g + 4, None, o, None) == INVALID
    assert lib.pw_stage_ext_dot(m, 8, 2, 8, g, g + 8, o, o) == INVALID
    assert lib.pw_stage_quotient_split(m + 4, 3, o) == INVALID
    assert (raw(torch, d_o) == SENT).all()
    abi.check(lib.pw_stage_ext_dot(m, 8, 2, 8, g, None, o, None), "pw_stage_ext_dot")
    abi.check(lib.pw_stage_row_layout(o, 3, 2, None, 0, 1, 0, 0), "pw_stage_row_layout")  # nothing asked for: nothing launched
    r = raw(torch, d_o)
    assert not (r[:8] == SENT).any() and (r[8:] == SENT).all()
