"""tests/_stage_ref.py (the reference the stage-kernel GPU tests compare with) held against things it did not define: the oracle's
extension field and transforms, polynomial identities (an opening IS an evaluation, a fold IS f_even + beta f_odd; the LogUp
permutation trace and the quotient satisfy the identity a verifier checks at a random point), and, for every vectorised routine, a
scalar twin in Python integers. No GPU."""
import numpy as np

from oracle import apc_model as om
from oracle import stark_model as sm
from tests import _stage_ref as ref
from tests._jit_host import eval_postfix

P = ref.P
EDGE_WORDS = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2]


def rand_ext(rng, n=None):
    return rng.integers(0, P, 4 if n is None else (n, 4), dtype=np.uint64)


def horner(coeffs, x):
    """sum_k c_k x^k for coefficients in F or E, x in E"""
    acc = ref.ZERO
    for c in reversed(list(coeffs)):
        acc = ref.ext_add(ref.ext_mul(acc, x), ref.ext(c))
    return acc


def as_tuples(a):
    return [tuple(int(x) for x in e) for e in np.asarray(a).reshape(-1, 4)]


def edge_elements(rng, n):
    return [tuple(int(x) for x in rng.choice(EDGE_WORDS, 4)) for _ in range(n)] + [(0, 1, 0, 0), (P - 1,) * 4, ref.ONE]


def test_extension_arithmetic_is_the_oracles():
    rng = np.random.default_rng(1)
    elems = as_tuples(rand_ext(rng, 20)) + edge_elements(rng, 30)
    for a in elems:
        for b in elems[::7]:
            assert ref.ext_mul(a, b) == tuple(sm.ext_mul(a, b).tolist()), (a, b)
        if a != ref.ZERO:
            assert ref.ext_inv(a) == tuple(sm.ext_inv(a).tolist()), a
            assert ref.ext_mul(a, ref.ext_inv(a)) == ref.ONE
    assert ref.ext_inv(ref.ZERO) == ref.ZERO and ref.inv(0) == 0


def test_domain_is_the_oracles_extended_domain():
    """the polynomial X, given by its values g^i, extends to x_j itself: the shift and the order of the rows are the oracle's"""
    for log_h in (1, 3, 6):
        got = sm.lde(ref.domain(log_h, 1).astype(np.uint32), 1, log_h)
        assert (got == ref.domain(log_h + 1)).all()
        assert int(got[0]) == ref.SHIFT
    assert pow(ref.root(5), 32, P) == 1 and pow(ref.root(5), 16, P) == P - 1 and ref.root(0) == 1


def test_opening_weights_open_a_polynomial():
    rng = np.random.default_rng(2)
    for log_h in (3, 6):
        H = 1 << log_h
        c = rng.integers(0, P, H, dtype=np.uint64)
        g = ref.domain(log_h, 1)
        evals = np.array([horner(c, ref.ext(int(x)))[0] for x in g], np.uint64)
        assert (sm.dft(evals.astype(np.uint32), inverse=True) == c).all()  # natural order, the oracle's root
        for zeta in as_tuples(rand_ext(rng, 3)) + [ref.ext(0), (P - 1,) * 4, (0, 1, 0, 0)]:
            want = horner(c, zeta)
            assert as_tuples(ref.ext_dot(evals[None, :], ref.barycentric_weights(zeta, log_h))) == [want], (log_h, zeta)
            # the layout of pw_lde_batch's d_coeffs: H c_bitrev(q)
            scaled = np.array([H * int(c[ref.bitrev(q, log_h)]) % P for q in range(H)], np.uint64)
            assert as_tuples(ref.ext_dot(scaled[None, :], ref.coefficient_weights(zeta, log_h))) == [want], (log_h, zeta)
        # a zeta inside the trace domain: the factor zeta^H - 1 vanishes, every weight is 0 (no division by zero is relied on)
        assert not ref.barycentric_weights(ref.ext(1), log_h).any()
        assert not ref.barycentric_weights(ref.ext(int(g[3])), log_h).any()
    assert as_tuples(ref.coefficient_weights((5, 6, 7, 8), 0)) == [ref.ONE]


def test_fri_fold_halves_a_polynomial():
    rng = np.random.default_rng(3)
    log_n = 4
    n = 1 << log_n
    f = as_tuples(rand_ext(rng, n))
    beta = tuple(int(x) for x in rand_ext(rng))
    folded = [ref.ext_add(fe, ref.ext_mul(beta, fo)) for fe, fo in zip(f[0::2], f[1::2])]  # f_even + beta f_odd
    for shift in (ref.SHIFT, 1):
        v = np.array([horner(f, ref.ext(int(x))) for x in ref.domain(log_n, shift)], np.uint64)
        want = [horner(folded, ref.ext(int(x))) for x in ref.domain(log_n - 1, shift * shift % P)]
        assert as_tuples(ref.fri_fold(v, log_n, shift, beta)) == want, shift


def test_vector_routines_equal_their_scalar_twins():
    rng = np.random.default_rng(4)
    a, b = rand_ext(rng, 40), rand_ext(rng, 40)
    a[:10] = np.array(edge_elements(rng, 7), np.uint64)
    assert as_tuples(ref.vmul(a, b)) == [ref.ext_mul(x, y) for x, y in zip(as_tuples(a), as_tuples(b))]
    assert as_tuples(ref.vadd(a, b)) == [ref.ext_add(x, y) for x, y in zip(as_tuples(a), as_tuples(b))]
    assert as_tuples(ref.vsub(a, b)) == [ref.ext_sub(x, y) for x, y in zip(as_tuples(a), as_tuples(b))]
    a[11] = 0
    assert as_tuples(ref.vext_inv(a)) == [ref.ext_inv(x) for x in as_tuples(a)]
    k = rng.integers(0, P, 40, dtype=np.uint64)
    k[:5] = EDGE_WORDS
    assert ref.vinv(k).tolist() == [ref.inv(int(x)) for x in k] and ref.vpow(k, 12345).tolist() == [pow(int(x), 12345, P) for x in k]
    assert as_tuples(ref.vscale(a, k)) == [ref.ext_scale(x, int(y)) for x, y in zip(as_tuples(a), k)]
    # sums over rows and columns
    log_n = 3
    N = 1 << log_n
    ma, mb = rng.integers(0, P, (3, N), dtype=np.uint64), rng.integers(0, P, (2, N), dtype=np.uint64)
    g = rand_ext(rng, 5)
    total, zeta = as_tuples(rand_ext(rng, 2))
    assert as_tuples(ref.lincomb(ma, g[:3])) == ref.lincomb_scalar(ma, g[:3])
    assert as_tuples(ref.deep(ma, mb, g, total, zeta, log_n)) == ref.deep_scalar(ma, mb, g, total, zeta, log_n)
    assert as_tuples(ref.ext_dot(ma, rand_ext(np.random.default_rng(5), N))) == ref.ext_dot_scalar(ma, rand_ext(np.random.default_rng(5), N))
    v = rand_ext(rng, 2 * N)
    assert as_tuples(ref.fri_fold(v, log_n + 1, 31 * 31, zeta)) == ref.fri_fold_scalar(v, log_n + 1, 31 * 31, zeta)
    assert ref.scan(v).tolist() == ref.scan_scalar(v)
    assert as_tuples(ref.ext_powers(zeta, 6)) == [ref.ext_pow(zeta, e) for e in range(6)]
    assert as_tuples(ref.ext_powers(zeta, 6, True)) == [ref.ext_pow(zeta, 5 - e) for e in range(6)]
    y = rand_ext(rng, 2 * N)
    assert as_tuples(ref.ext_axpy(y, zeta, v)) == [ref.ext_add(p, ref.ext_mul(zeta, q)) for p, q in zip(as_tuples(y), as_tuples(v))]
    assert as_tuples(ref.ext_axpy(y, None, v)) == as_tuples(ref.vadd(y, v))


def test_two_term_deep_forms_agree():
    """deep_logup written out row by row with Python integers; the route over ext_lincomb + deep_from_combo gives the same vector"""
    rng = np.random.default_rng(6)
    log_n, W, Wp = 2, 3, 5
    N, K1 = 1 << log_n, W + Wp + 8
    lde, plde, qlde = (rng.integers(0, P, (w, N), dtype=np.uint64) for w in (W, Wp, 8))
    g = rand_ext(rng, K1 + Wp)
    gt = as_tuples(g)
    sum1, sum2, zeta, gzeta, gK = as_tuples(rand_ext(rng, 5))
    x = ref.domain(log_n)
    for two_point in (False, True):
        want = []
        for j in range(N):
            row = ref.lincomb_scalar(lde[:, j:j + 1], gt[:W])[0]
            a1 = ref.ext_add(ref.ext_add(row, ref.lincomb_scalar(plde[:, j:j + 1], gt[W:W + Wp])[0]),
                             ref.lincomb_scalar(qlde[:, j:j + 1], gt[W + Wp:K1])[0])
            a2 = ref.lincomb_scalar(plde[:, j:j + 1], gt[K1:])[0]
            if two_point:
                a2 = ref.ext_add(a2, ref.ext_mul(gK, row))
            xe = ref.ext(int(x[j]))
            want.append(ref.ext_add(ref.ext_mul(ref.ext_sub(a1, sum1), ref.ext_inv(ref.ext_sub(xe, zeta))),
                                    ref.ext_mul(ref.ext_sub(a2, sum2), ref.ext_inv(ref.ext_sub(xe, gzeta)))))
        assert as_tuples(ref.deep_logup(lde, plde, qlde, g, sum1, sum2, zeta, gzeta, log_n, gK if two_point else None)) == want
    combo = ref.ext_lincomb(lde, plde, g, K1)
    assert combo.shape == (8, N) and ref.ext_lincomb(lde, plde, g, 0).shape == (4, N)
    assert (ref.deep_from_combo(combo, qlde, g[W + Wp:K1], sum1, sum2, zeta, gzeta, True, log_n)
            == ref.deep_logup(lde, plde, qlde, g, sum1, sum2, zeta, gzeta, log_n)).all()
    # without the second term: the first quotient alone, i.e. deep over (lde | plde | qlde) with the first K1 powers
    assert (ref.deep_from_combo(combo, qlde, g[W + Wp:K1], sum1, sum2, zeta, gzeta, False, log_n)
            == ref.deep(np.concatenate([lde, plde]), qlde, g[:K1], sum1, zeta, log_n)).all()


def test_small_kernels_equal_their_formulas():
    rng = np.random.default_rng(7)
    # quotient_split
    log_h = 3
    H = 1 << log_h
    cbr = rng.integers(0, P, (4, 2 * H), dtype=np.uint64)
    got = ref.quotient_split(cbr, log_h)
    sinv = ref.inv(ref.SHIFT)
    for ch in range(2):
        for k in range(4):
            for q in range(H):
                assert int(got[4 * ch + k, q]) == int(cbr[k, 2 * q + ch]) * pow(sinv, ref.bitrev(q, log_h) + ch * H, P) * ref.inv(2) % P
    assert ref.quotient_split(cbr[:, :2], 0).tolist() == [[int(cbr[k, 0]) * ref.inv(2) % P] for k in range(4)] + \
        [[int(cbr[k, 1]) * sinv * ref.inv(2) % P] for k in range(4)]
    # row_layout: shifted columns, and the selectors through the identities that define them
    log_n = 3
    n = 1 << log_n
    m = rng.integers(0, P, (4, n), dtype=np.uint64)
    for trace_domain in (False, True):
        for step in (1, 2):
            out = ref.row_layout(m, log_n, [2, 0, 2], step, True, trace_domain)
            assert out.shape == (6, n)
            for i, c in enumerate([2, 0, 2]):
                assert [int(out[i, j]) for j in range(n)] == [int(m[c, (j + step) % n]) for j in range(n)]
            w = ref.root(log_n)
            Hh, g, s = (n, w, 1) if trace_domain else (n // 2, w * w % P, ref.SHIFT)
            ginv = ref.inv(g)
            for j in range(n):
                x = s * pow(w, j, P) % P
                z = (pow(x, Hh, P) - 1) % P
                first, last, trans = (int(out[3 + t, j]) for t in range(3))
                assert trans == (x - ginv) % P
                assert first * (x - 1) % P == z and last * (x - ginv) % P == z
                if trace_domain:  # Z_H = 0 on every row: the products above say nothing at the roots themselves
                    assert first == (Hh if j == 0 else 0) and last == (Hh * g % P if j == n - 1 else 0)
                    # the quotient polynomial's value at its root: (x^H - 1) / (x - 1) = 1 + x + ... + x^(H-1)
                    assert sum(pow(x, e, P) for e in range(Hh)) % P == first
        assert ref.row_layout(m, log_n, [], 1, False, trace_domain).shape == (0, n)
        assert ref.row_layout(m, log_n, [1], 1, False, trace_domain).shape == (1, n)
    # Z_H(x) / (x - g^-1) at x = g^-1 on the trace domain: sum_e x^e g^-(H-1-e) = H x^(H-1) = H g
    assert int(ref.row_layout(m, log_n, [], 1, True, True)[1, n - 1]) == n * pow(ref.inv(ref.root(log_n)), n - 1, P) % P
    # part_scatter
    part = rng.integers(0, P, (3, 4, 5), dtype=np.uint64)
    b, r, N = 2, 3, 24
    before = rng.integers(0, P, (4, N), dtype=np.uint64)
    got = ref.part_scatter(part, b, r, before)
    want = before.copy()
    for k in range(4):
        for i in range(5):
            want[k, r + (i << b)] = sum(int(part[c, k, i]) for c in range(3)) % P
    assert (got == want).all()


def test_centred_encoding_round_trips():
    rng = np.random.default_rng(8)
    c = np.concatenate([rng.integers(0, P, 1000, dtype=np.uint64), np.array(EDGE_WORDS, np.uint64), ref.from_word(np.array(EDGE_WORDS, np.uint64))])
    t = ref.centred_encode(c)
    assert t.dtype == np.int32 and (np.abs(t.astype(np.int64)) <= ref.HALF).all()
    assert (ref.centred_decode(t) == c).all()
    assert ((t.astype(np.int64) - ref.to_word(c).astype(np.int64)) % P == 0).all()
    # the two neighbours of p / 2, as WORDS
    assert ref.centred_encode(ref.from_word(np.array([(P - 1) // 2, (P + 1) // 2], np.uint64))).tolist() == [ref.HALF, -ref.HALF]
    # and the oracle's Montgomery conversion is the one used here
    assert (om.to_monty(c.astype(np.uint32)) == ref.to_word(c)).all() and (om.from_monty(c.astype(np.uint32)) == ref.from_word(c)).all()


# ---------------------------------------------------------------------------------------------------------------- LogUp and the quotient
class E:
    """an extension element with operators: what eval_postfix needs to run a program on OPENINGS (cells in E); Python integers only"""

    def __init__(self, v):
        self.v = v.v if isinstance(v, E) else ref.ext(v)

    __add__ = __radd__ = lambda a, b: E(ref.ext_add(a.v, E(b).v))
    __mul__ = __rmul__ = lambda a, b: E(ref.ext_mul(a.v, E(b).v))
    __sub__ = lambda a, b: E(ref.ext_sub(a.v, E(b).v))
    __rsub__ = lambda a, b: E(ref.ext_sub(E(b).v, a.v))
    __neg__ = lambda a: E(ref.ext_sub(ref.ZERO, a.v))
    __mod__ = lambda a, _p: a
    __eq__ = lambda a, b: a.v == E(b).v


X = E((0, 1, 0, 0))


def from_coordinates(cols4):
    """four openings of coordinate columns -> the opening of the extension-valued column: sum_k X^k c_k"""
    return cols4[0] + X * (cols4[1] + X * (cols4[2] + X * cols4[3]))


def folded_combination(cells, perm, perm_next, selectors, cons, it, starts, apow, alpha, blpow, S):
    """sum_c apow[c] C_c + sum_g apow[nc + g] (q_g den_g - num_g) + apow[nc + G] is_first (phi - sum q) + apow[nc + G + 1]
    is_transition (phi' - phi - sum q') + apow[nc + G + 2] is_last (phi - S), from ONE point's values (a trace row or the openings at
    zeta and g zeta), scalar by scalar: cells (W), perm / perm_next (4 G + 4 coordinate values at the point and at its successor),
    selectors = (is_first, is_last, is_transition). -> (the combination, [q_g den_g - num_g per group])"""
    (bc, spans), (inter, ispans, ibc) = cons, it
    prog = lambda code, s: eval_postfix(code[int(s[0]):int(s[0]) + int(s[1])].tolist(), cells)
    nc, G = len(spans), len(starts) - 1
    acc = E(0)
    for c in range(nc):
        acc = acc + E(apow[c]) * prog(bc, spans[c])
    ms, ds = [], []
    for bus, n_args, s0 in inter.tolist():
        ms.append(E(prog(ibc, ispans[s0])))
        d = E(alpha) + bus
        for j in range(n_args):
            d = d + E(blpow[j + 1]) * prog(ibc, ispans[s0 + 1 + j])
        ds.append(d)
    terms, sumq, sumq_next = [], E(0), E(0)
    for g in range(G):
        members = range(int(starts[g]), int(starts[g + 1]))
        den, num = E(1), E(0)
        for i in members:
            den = den * ds[i]
            rest = E(1)
            for l in members:
                if l != i:
                    rest = rest * ds[l]
            num = num + ms[i] * rest
        qg = from_coordinates(perm[4 * g:4 * g + 4])
        terms.append(qg * den - num)
        acc = acc + E(apow[nc + g]) * terms[-1]
        sumq, sumq_next = sumq + qg, sumq_next + from_coordinates(perm_next[4 * g:4 * g + 4])
    phi, phi_next = from_coordinates(perm[4 * G:4 * G + 4]), from_coordinates(perm_next[4 * G:4 * G + 4])
    is_first, is_last, is_trans = selectors
    acc = acc + E(apow[nc + G]) * (is_first * (phi - sumq))
    acc = acc + E(apow[nc + G + 1]) * (is_trans * (phi_next - phi - sumq_next))
    acc = acc + E(apow[nc + G + 2]) * (is_last * (phi - E(S)))
    return acc, terms


def test_logup_and_quotient_references_satisfy_the_verifiers_identity():
    """A small AIR whose trace satisfies its constraints and whose bus balances: the reference's permutation trace and quotient, with
    true powers of random challenges, satisfy what a verifier checks — at a random point zeta of E the folded combination of the
    openings (trace and permutation matrix at zeta and g zeta, recomputed here scalar by scalar) equals Z_H(zeta) q(zeta); on the
    trace domain every group's q_g den_g - num_g vanishes, and phi's differences are the row sums."""
    from tests import _random_airs as ra

    for seed in (1, 2, 3):
        log_h = 4
        H, N, log_n = 1 << log_h, 2 << log_h, log_h + 1
        air = ra.derived_air(seed, log_h)
        W, cons, it, T = air["W"], air["cons"], air["it"], air["T"]
        assert air["check"](T)[0] == 0
        starts = sm.group_starts(*it)
        nc, G = len(cons[1]), len(starts) - 1
        rng = np.random.default_rng(100 + seed)
        alpha, beta, alpha_c, zeta = as_tuples(rand_ext(rng, 4))
        blpow = ref.ext_powers(beta, int(it[0][:, 1].max()) + 2)
        apow = ref.ext_powers(alpha_c, nc + G + 3, reversed_=True)
        q, rowsum, phi = ref.logup_perm(T, it, starts, alpha, blpow)
        assert q.shape == (G, H, 4) and as_tuples(phi[0]) == as_tuples(rowsum[0])
        for r in range(1, H):
            assert ref.ext_sub(as_tuples(phi[r])[0], as_tuples(phi[r - 1])[0]) == as_tuples(rowsum[r])[0]
        S = as_tuples(phi[H - 1])[0]
        assert S == ref.ZERO  # the bus balances
        perm = np.concatenate([q.transpose(0, 2, 1).reshape(4 * G, H), phi.T]).astype(np.uint32)
        # on the trace domain: the group terms vanish row by row, the boundary terms too (the selectors' values there: row_layout)
        sel = ref.row_layout(np.zeros((0, H), np.uint64), log_h, [], 1, True, True)
        for r in range(H):
            nxt = (r + 1) % H
            acc, terms = folded_combination([E(int(x)) for x in T[:, r]], [E(int(x)) for x in perm[:, r]], [E(int(x)) for x in perm[:, nxt]],
                                            [E(int(sel[t, r])) for t in range(3)], cons, it, starts, as_tuples(apow), alpha, as_tuples(blpow), S)
            assert all(t == 0 for t in terms) and acc == 0, (seed, r)
        lde = sm.lde(T.reshape(-1), W, log_h).reshape(W, N)
        plde = sm.lde(perm.reshape(-1), 4 * G + 4, log_h).reshape(4 * G + 4, N)
        quot = ref.quotient(lde, plde, log_n, cons, it, starts, apow, alpha, blpow, S)
        # openings
        g = ref.root(log_h)
        gzeta = ref.ext_scale(zeta, g)
        w, w_next = ref.barycentric_weights(zeta, log_h), ref.barycentric_weights(gzeta, log_h)
        cells = [E(e) for e in as_tuples(ref.ext_dot(T, w))]
        p_z, p_gz = [E(e) for e in as_tuples(ref.ext_dot(perm, w))], [E(e) for e in as_tuples(ref.ext_dot(perm, w_next))]
        # the quotient's interpolant over the shifted domain: v_j = sum_k c_k s^k w^(jk), so the inverse DFT gives c_k s^k
        sinv = ref.inv(ref.SHIFT)
        q_z = []
        for k in range(4):
            cs = sm.dft(quot[:, k].astype(np.uint32), inverse=True)
            c = [int(cs[i]) * pow(sinv, i, P) % P for i in range(N)]
            scaled = np.array([N * c[ref.bitrev(i, log_n)] % P for i in range(N)], np.uint64)
            q_z.append(E(as_tuples(ref.ext_dot(scaled[None, :], ref.coefficient_weights(zeta, log_n)))[0]))
        z_h = E(ref.ext_pow(zeta, H)) - 1
        ginv = ref.inv(g)
        selectors = (z_h * E(ref.ext_inv(ref.ext_sub(zeta, ref.ONE))), z_h * E(ref.ext_inv(ref.ext_sub(zeta, ref.ext(ginv)))), E(zeta) - ginv)
        acc, _ = folded_combination(cells, p_z, p_gz, selectors, cons, it, starts, as_tuples(apow), alpha, as_tuples(blpow), S)
        assert acc == z_h * from_coordinates(q_z), seed
        # the unscaled current-row part is the quotient's own first two sums
        sums = ref.quotient_sums(lde, plde, cons, it, starts, apow, alpha, blpow)
        assert (ref.logup_tail(sums.T[None], plde[4 * G:], plde[:4 * G].reshape(G, 4, N).sum(axis=0) % P, log_n, apow[nc + G:], S) == quot).all()
        # constraints only: C / Z_H, a polynomial of degree < N again
        quot0 = ref.quotient(lde, None, log_n, cons, None, None, apow)
        c0 = E(0)
        for c in range(nc):
            off, ln = cons[1][c]
            c0 = c0 + E(as_tuples(apow)[c]) * eval_postfix(cons[0][int(off):int(off) + int(ln)].tolist(), cells)
        q0_z = []
        for k in range(4):
            cs = sm.dft(quot0[:, k].astype(np.uint32), inverse=True)
            q0_z.append(E(horner([int(cs[i]) * pow(sinv, i, P) % P for i in range(N)], zeta)))
        assert c0 == z_h * from_coordinates(q0_z), seed


def test_a_vanishing_denominator_zeroes_its_group_and_is_reported_elsewhere():
    """1 / 0 = 0 for the group's ONE inversion; a denominator that vanishes where the caller did not say so is an error of the inputs"""
    import pytest

    from tests._edge_values import PA, PC, _programs

    _, it = _programs([], [(3, [PC, 1], [[PA, 0]]), (3, [PA, 1], [[PC, 5]]), (4, [PC, 2], [[PA, 2]])])
    starts = sm.group_starts(*it)
    rng = np.random.default_rng(9)
    T = rng.integers(1, P, (3, 8), dtype=np.uint64)
    beta = as_tuples(rand_ext(rng))[0]
    blpow = ref.ext_powers(beta, 3)
    alpha = ref.ext_sub(ref.ZERO, ref.ext_add(ref.ext(3), ref.ext_scale(beta, int(T[0, 5]))))  # d_0 = 0 on row 5
    with pytest.raises(AssertionError):
        ref.logup_perm(T, it, starts, alpha, blpow)
    q, rowsum, _ = ref.logup_perm(T, it, starts, alpha, blpow, vanishing=[(0, 5)])
    g0 = [g for g in range(len(starts) - 1) if starts[g] <= 0 < starts[g + 1]][0]
    assert not q[g0, 5].any() and q[g0, 4].any()
    ms, ds = ref.interaction_values(T, it, alpha, blpow)
    for g in range(len(starts) - 1):
        for r in (4, 5):
            want = ref.ZERO
            if not (g == g0 and r == 5):
                for i in range(int(starts[g]), int(starts[g + 1])):
                    want = ref.ext_add(want, ref.ext_scale(ref.ext_inv(as_tuples(ds[i][r])[0]), int(ms[i][r])))
            assert as_tuples(q[g, r])[0] == want, (g, r)


def test_inputs_of_the_logup_stage_tests_are_what_they_claim():
    """tests/test_stage_logup_gpu.py's AIRs and input families, without a GPU: the column AIR's groups; the jit-small chunking yields
    several chunks and units; in every family of every permutation-trace case no denominator vanishes (logup_perm asserts it), in the
    vanishing-denominator cases exactly the planted one does, where every multiplicity of its group is non-zero; the bound families put
    the extreme words where they say"""
    from powdr_amd import prover
    from tests import test_stage_logup_gpu as t

    W, cons, it = t.column_air()
    starts = t.group_starts(it)
    assert [b - a for a, b in zip(starts, starts[1:])] == [3, 2, 2, 2, 1] and (prover.logup_group_starts(it) == starts).all()
    assert sorted(set(it[0][:, 1].tolist())) == [0, 1, 2, 3, 4, 5, 7] and len(cons[1]) >= 5
    assert len(t.wide_air()[1][1]) >= 64
    for name, make in t.AIRS.items():
        W, cons, it = make()
        units, total = prover.jit_generated_sources(W, cons[0], cons[1], it, 0, 200, 1)
        n_perm = prover.jit_generated_sources(W, cons[0], cons[1], it, 1, 200, 1)[1] if it is not None else 0
        assert total + n_perm >= 3 and len(units) >= 2, (name, total, n_perm)
    assert int(om.to_monty(np.array([t.PM1, t.WORD_HI, t.WORD_LO], np.uint32))[0]) == P - 1
    assert ref.centred_encode(np.array([t.WORD_HI, t.WORD_LO], np.uint64)).tolist() == [ref.HALF, -ref.HALF]
    for name in ("hand", "column"):
        W, cons, it = t.AIRS[name]()
        starts = t.group_starts(it)
        for log_h in (1, 2, 8, 9):
            for family in t.PERM_FAMILIES[name]:
                rng = np.random.default_rng([1, log_h, t.PERM_FAMILIES["column"].index(family)])
                T, alpha, blpow = t.perm_inputs(name, family, rng, W, it, log_h)
                q, rowsum, _ = ref.logup_perm(T, it, starts, alpha, blpow)
                assert q.any() and (log_h < 8 or name == "hand" or not rowsum[3].any())  # row 3: every multiplicity column is zero
        for log_h in (1, 9):
            T, alpha, blpow, i, rows = t.vanishing_inputs(name, np.random.default_rng([2, log_h]), W, it, log_h)
            ref.logup_perm(T, it, starts, alpha, blpow, vanishing=[(i, r) for r in rows])
            ms, ds = ref.interaction_values(T, it, alpha, blpow)
            assert not ds[i][rows].any() and all(int(m[r]) for m in ms for r in rows)


# ---- the query phase -------------------------------------------------------------------------------------------------------------------
def numpy_pow_search(state, pending, bits, n, constants):
    """the kernel's shortcut, restated: the pending words and the candidate overwrite the state, ONE permutation, word 7, its low bits"""
    from tests import _poseidon2_air_ref as p2

    st = np.tile(np.asarray(state, np.int64), (n, 1))
    st[:, :len(pending)] = np.asarray(pending, np.int64)
    st[:, len(pending)] = np.arange(n)
    word7 = p2.permute(st, constants)[0][:, 7]
    return [next((int(w) for w in np.nonzero((word7 & ((1 << b) - 1)) == 0)[0]), sm.POW_NONE) for b in bits]


def test_pow_witness_observes_and_samples_like_one_overwrite_and_one_permutation():
    """or_pow_witness grinds with the oracle's Challenger (copy, observe, sample_bits); for every in_len — the witness fills the rate
    at 7, a sample forces the duplex below — that is the overwrite / permute / word 7 rule pow_kernel uses"""
    constants = sm.poseidon2_constants()
    bits, n = [1, 2, 4, 7, 8], 1 << 12
    for name, (state, pending) in ref.pow_families(np.random.default_rng(200)).items():
        for in_len in range(8):
            want = numpy_pow_search(state, pending[:in_len], bits, n, constants)
            got = [sm.pow_witness(state, pending[:in_len], b, 0, n) for b in bits]
            assert got == want, (name, in_len, got, want)
            assert want[0] != sm.POW_NONE and want[2] != sm.POW_NONE  # 2^12 candidates: a miss at 4 bits has probability e^-256
            w = want[4]
            if w != sm.POW_NONE and w > 0:  # the range is half-open on both sides of the witness
                assert sm.pow_witness(state, pending[:in_len], 8, 0, w) == sm.POW_NONE
                assert sm.pow_witness(state, pending[:in_len], 8, w, w + 1) == w
                assert sm.pow_witness(state, pending[:in_len], 8, w + 1, n) == numpy_pow_search_from(state, pending[:in_len], 8, w + 1, n, constants)
    s, q = np.zeros(16, np.uint32), np.zeros(7, np.uint32)
    bad = s.copy()
    bad[3] = P
    assert sm.pow_witness(bad, q, 4) == sm.POW_NONE and sm.pow_witness(s, np.full(3, P, np.uint32), 4) == sm.POW_NONE
    assert sm.pow_witness(s, q, 0) == sm.POW_NONE and sm.pow_witness(s, q, 32) == sm.POW_NONE
    assert sm.pow_witness(s, np.zeros(8, np.uint32), 4) == sm.POW_NONE and sm.pow_witness(s, q, 4, 5, 5) == sm.POW_NONE


def numpy_pow_search_from(state, pending, bits, lo, n, constants):
    from tests import _poseidon2_air_ref as p2

    st = np.tile(np.asarray(state, np.int64), (n - lo, 1))
    st[:, :len(pending)] = np.asarray(pending, np.int64)
    st[:, len(pending)] = np.arange(lo, n)
    hits = np.nonzero((p2.permute(st, constants)[0][:, 7] & ((1 << bits) - 1)) == 0)[0]
    return lo + int(hits[0]) if len(hits) else sm.POW_NONE


def test_lde_rows_are_the_oracles_extension():
    """values -> coefficients by the oracle's inverse DFT -> every row of the oracle's LDE, log_h 1 .. 6; and the device layout of the
    coefficients: H c_bitrev(q), which the coefficient weights open at any point"""
    rng = np.random.default_rng(201)
    for log_h in range(1, 7):
        H, W = 1 << log_h, 3
        values = rng.integers(0, P, (W, H), dtype=np.uint32)
        values[1] = P - 1
        c = np.stack([sm.dft(v, inverse=True) for v in values])
        want = sm.lde(values.reshape(-1), W, log_h).reshape(W, 2 * H).T
        idx = list(range(2 * H))
        assert (ref.lde_rows(c, log_h, idx) == want).all(), log_h
        assert (ref.lde_rows(c, log_h, idx[::-1] + [0, 0]) == np.concatenate([want[::-1], want[:1], want[:1]])).all()
        arrays = ref.coefficient_arrays(c, log_h)
        for col in range(W):
            idft = sm.dft(values[col], inverse=True)
            assert arrays[col].tolist() == [H * int(idft[ref.bitrev(q, log_h)]) % P for q in range(H)]
        zeta = tuple(int(x) for x in rng.integers(0, P, 4))
        assert as_tuples(ref.ext_dot(arrays, ref.coefficient_weights(zeta, log_h))) == [horner(col, zeta) for col in c]
    x = 123456789
    assert ref.power_vector(x, 64).tolist() == [pow(x, k, P) for k in range(64)] and ref.power_vector(x, 1).tolist() == [1]


def test_gathers_and_the_transpose_are_plain_indexing():
    m = np.arange(15, dtype=np.uint32).reshape(3, 5)
    assert ref.gather_rows(m, [4, 0, 4]).tolist() == [[4, 9, 14], [0, 5, 10], [4, 9, 14]]
    assert ref.gather_records(np.arange(40), [8, 0, 8], 4).tolist() == [[8, 9, 10, 11], [0, 1, 2, 3], [8, 9, 10, 11]]
    assert ref.ext_to_cols(np.arange(12)).tolist() == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
