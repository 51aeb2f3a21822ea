"""A plain reference of the opening, DEEP, FRI, scan and layout stages (csrc/stark_kernels.hip, logup_kernels.hip, stream_kernels.hip),
one function per stage, each stating the formula of the kernel's comment. Pure Python and numpy, no library call; importable without a
GPU. Everything here is a CANONICAL value; the prime, the roots of unity and the coset shift are the oracle's. The extension is
E = F[X] / (X^4 - 11), an element = 4 coordinates, lowest degree first.

Two layers. Scalars (a challenge, an opened sum, one weight) are tuples of 4 Python integers: ext_add .. ext_pow. Whole vectors are
numpy uint64 arrays with a last axis of 4 (v*): every product of two words below p is below 2^62 and is reduced at once, a sum of 2^14
reduced words is below 2^45, so uint64 never wraps (the longest sums here: 16384 rows in ext_dot, 65536 in the scan — below 2^47).
tests/test_stage_ref_cpu.py holds the scalar layer against the oracle's field and against polynomial identities, and every v* routine
against its scalar twin.

The stage in front of those — the LogUp permutation trace and the quotient (logup_perm, quotient_sums, quotient, logup_tail,
rowsum_combine) — is here too, over the post-fix evaluator of tests/_jit_host.py; test_stage_ref_cpu.py holds it to the identity a
verifier checks at a random point, recomputed there scalar by scalar."""
import functools

import numpy as np

from oracle import apc_model as om
from oracle import stark_model as sm

P = om.P
SHIFT = 31  # the coset shift s (oracle/stark_oracle.cpp COSET_SHIFT; test_stage_ref_cpu.py reads it back out of the oracle's LDE)
W11 = 11    # X^4 = 11
HALF = (P - 1) // 2
_R = (1 << 32) % P
_RINV = pow(_R, -1, P)
_p = np.uint64(P)


# ---------------------------------------------------------------------------------------------------------- the base field
def inv(a: int) -> int:
    """a^(p-2); 0 for 0, as the kernels' Fermat inverse"""
    return pow(a % P, P - 2, P)


@functools.lru_cache(maxsize=None)
def root(log_n: int) -> int:
    """the oracle's generator of the order-2^log_n subgroup"""
    return sm.root_of_unity(log_n)


def bitrev(q: int, bits: int) -> int:
    r = 0
    for _ in range(bits):
        r, q = (r << 1) | (q & 1), q >> 1
    return r


@functools.lru_cache(maxsize=None)
def domain(log_n: int, shift: int = SHIFT):
    """x_j = shift * w^j, j < 2^log_n, w = root(log_n): a uint64 array"""
    w, x, out = root(log_n), shift % P, []
    for _ in range(1 << log_n):
        out.append(x)
        x = x * w % P
    a = np.array(out, np.uint64)
    a.setflags(write=False)
    return a


def vpow(a, e: int):
    """a^e element by element (square and multiply over the bits of e)"""
    a = np.asarray(a, np.uint64) % _p
    r = np.ones_like(a)
    while e:
        if e & 1:
            r = r * a % _p
        a = a * a % _p
        e >>= 1
    return r


def vinv(a):
    return vpow(a, P - 2)


# ---------------------------------------------------------------------------------------------------------- E, scalars
ZERO, ONE = (0, 0, 0, 0), (1, 0, 0, 0)


def ext(a):
    """a base-field integer or 4 coordinates -> a tuple of 4 Python integers in [0, p)"""
    if isinstance(a, (int, np.integer)):
        return (int(a) % P, 0, 0, 0)
    t = tuple(int(x) % P for x in a)
    assert len(t) == 4
    return t


def ext_add(a, b):
    return tuple((x + y) % P for x, y in zip(a, b))


def ext_sub(a, b):
    return tuple((x - y) % P for x, y in zip(a, b))


def ext_scale(a, k: int):
    return tuple(x * k % P for x in a)


def ext_mul(a, b):
    """the product of two cubics, X^(4 + i) = 11 X^i"""
    c = [0] * 7
    for i in range(4):
        for j in range(4):
            c[i + j] += a[i] * b[j]
    return tuple((c[i] + (W11 * c[i + 4] if i < 3 else 0)) % P for i in range(4))


def ext_pow(a, e: int):
    r = ONE
    while e:
        if e & 1:
            r = ext_mul(r, a)
        a = ext_mul(a, a)
        e >>= 1
    return r


def ext_inv(a):
    """a^(p^4 - 2): the multiplicative group of E has p^4 - 1 elements; 0 for 0"""
    return ext_pow(a, P ** 4 - 2)


# ---------------------------------------------------------------------------------------------------------- E, vectors
def vext(a):
    """anything of shape (..., 4) -> uint64, reduced"""
    a = np.asarray(a)
    assert a.shape[-1] == 4
    return (a.astype(np.int64) % P).astype(np.uint64) if a.dtype.kind == "i" else a.astype(np.uint64) % _p


def vadd(a, b):
    return (vext(a) + vext(b)) % _p


def vsub(a, b):
    return (vext(a) + _p - vext(b)) % _p


def vscale(a, k):
    """a (..., 4) times base-field words k (...)"""
    return vext(a) * (np.asarray(k, np.uint64) % _p)[..., None] % _p


def vmul(a, b):
    """element by element (broadcasting); every product is reduced before it is added: at most 4 terms below p, and 11 times 3"""
    a, b = vext(a), vext(b)
    m = lambda i, j: a[..., i] * b[..., j] % _p
    w = np.uint64(W11)
    c0 = (m(0, 0) + w * (m(1, 3) + m(2, 2) + m(3, 1))) % _p
    c1 = (m(0, 1) + m(1, 0) + w * (m(2, 3) + m(3, 2))) % _p
    c2 = (m(0, 2) + m(1, 1) + m(2, 0) + w * m(3, 3)) % _p
    c3 = (m(0, 3) + m(1, 2) + m(2, 1) + m(3, 0)) % _p
    return np.stack([c0, c1, c2, c3], axis=-1)


def vext_inv(a):
    """element by element through the quadratic subfield K = F[Y] / (Y^2 - 11), Y = X^2: a = A0 + A1 X with A0 = a0 + a2 Y and
    A1 = a1 + a3 Y, a (A0 - A1 X) = A0^2 - Y A1^2 = D in K, and D (d0 - d1 Y) = d0^2 - 11 d1^2 in F. (The scalar ext_inv is a plain
    power instead; test_stage_ref_cpu.py holds the two against each other.) 0 for 0."""
    a = vext(a)
    a0, a1, a2, a3 = (a[..., i] for i in range(4))
    w = np.uint64(W11)
    mul = lambda x, y: x * y % _p
    kmul = lambda x0, x1, y0, y1: ((mul(x0, y0) + w * mul(x1, y1)) % _p, (mul(x0, y1) + mul(x1, y0)) % _p)  # (x0 + x1 Y)(y0 + y1 Y)
    s0, s1 = kmul(a0, a2, a0, a2)  # A0^2
    t0, t1 = kmul(a1, a3, a1, a3)  # A1^2;  Y (t0 + t1 Y) = 11 t1 + t0 Y
    d0, d1 = (s0 + _p - w * t1 % _p) % _p, (s1 + _p - t0) % _p
    ni = vinv((mul(d0, d0) + _p - w * mul(d1, d1) % _p) % _p)
    e0, e1 = mul(d0, ni), (_p - mul(d1, ni)) % _p  # 1 / D
    r0, r2 = kmul(a0, a2, e0, e1)  # A0 / D
    n1, n3 = kmul(a1, a3, e0, e1)  # A1 / D, to be negated
    return np.stack([r0, (_p - n1) % _p, r2, (_p - n3) % _p], axis=-1)


# ---------------------------------------------------------------------------------------------------------- the table form
def to_word(c):
    """canonical -> Montgomery word (c 2^32 mod p)"""
    return np.asarray(c, np.uint64) % _p * np.uint64(_R) % _p


def from_word(w):
    return np.asarray(w, np.uint64) % _p * np.uint64(_RINV) % _p


def centred_encode(c):
    """canonical values -> the int32 the weight and gamma tables hold: the representative of the MONTGOMERY word in
    [-(p-1)/2, (p-1)/2] (bb::centred: a word above p / 2 goes to word - p)"""
    w = to_word(c).astype(np.int64)
    return np.where(w > HALF, w - P, w).astype(np.int32)


def centred_decode(t):
    """any int32 table (|.| <= (p-1)/2, produced by a kernel or not) -> the canonical values it stands for"""
    return from_word((np.asarray(t, np.int64) % P).astype(np.uint64))


# ---------------------------------------------------------------------------------------------------------- opening weights
def barycentric_weights(zeta, log_h: int):
    """w_i = ((zeta^H - 1) / H) g^i / (zeta - g^i), i < H, g = root(log_h): f(zeta) = sum_i f(g^i) w_i for deg f < H. A zeta INSIDE the
    trace domain has zeta^H = 1: the factor in front is 0 and (with 1 / 0 = 0, as the kernels' inverse) every weight is 0."""
    zeta = ext(zeta)
    H = 1 << log_h
    scale = ext_scale(ext_sub(ext_pow(zeta, H), ONE), inv(H))
    g = domain(log_h, 1)
    den = vsub(np.array(zeta, np.uint64)[None, :], np.stack([g, 0 * g, 0 * g, 0 * g], axis=-1))
    return vmul(vscale(np.array(scale, np.uint64)[None, :], g), vext_inv(den))


def coefficient_weights(zeta, log_h: int):
    """w[q] = zeta^bitrev(q) / H, for coefficient arrays in bit-reversed order that carry a factor H (pw_lde_batch's
    d_coeffs[q] = H c_bitrev(q)): sum_q d_coeffs[q] w[q] = sum_k c_k zeta^k = f(zeta)"""
    zeta = ext(zeta)
    H = 1 << log_h
    hinv, pw, x = inv(H), [], ONE
    for _ in range(H):
        pw.append(ext_scale(x, hinv))
        x = ext_mul(x, zeta)
    return np.array([pw[bitrev(q, log_h)] for q in range(H)], np.uint64)


def ext_dot(cols, w, w2=None):
    """out_c = sum_q w(q) col_c(q): cols (n_cols, len) words, w (len, 4) -> (n_cols, 4); with w2 a pair of them. Per coordinate the
    products are reduced one by one, then up to 16384 of them (< 2^45) are added."""
    cols = np.asarray(cols, np.uint64)
    one = lambda wv: np.stack([(cols * vext(wv)[None, :, k] % _p).sum(axis=1) % _p for k in range(4)], axis=-1)
    return one(w) if w2 is None else (one(w), one(w2))


def ext_powers(base, n: int, reversed_: bool = False):
    """out[k] = base^k, or base^(n - 1 - k) when reversed; n successive multiplications"""
    base, out, x = ext(base), [], ONE
    for _ in range(n):
        out.append(x)
        x = ext_mul(x, base)
    return np.array(out[::-1] if reversed_ else out, np.uint64).reshape(n, 4)


# ---------------------------------------------------------------------------------------------------------- DEEP
def lincomb(m, g):
    """sum_k g[k] m_k as a vector of E: m (w, n) words, g (w, 4) -> (n, 4); w = 0 gives zeros"""
    m, g = np.asarray(m, np.uint64), vext(g)
    assert len(m) == len(g)
    return np.stack([(m * g[:, k, None] % _p).sum(axis=0) % _p for k in range(4)], axis=-1)


@functools.lru_cache(maxsize=None)
def _inv_den(log_n: int, point):
    """1 / (x_j - point), j < 2^log_n, on the extended domain x_j = s w^j"""
    x = domain(log_n)
    r = vext_inv(vsub(np.stack([x, 0 * x, 0 * x, 0 * x], axis=-1), np.array(point, np.uint64)[None, :]))
    r.setflags(write=False)
    return r


def _quotient(num, total, log_n, point):
    return vmul(vsub(num, np.array(ext(total), np.uint64)[None, :]), _inv_den(log_n, ext(point)))


def deep(a, b, g, total, zeta, log_n: int):
    """v_j = (sum_k g_k a_k(x_j) + sum_k g_(wa + k) b_k(x_j) - total) / (x_j - zeta); a (wa, N), b (wb, N), g (wa + wb, 4)"""
    return _quotient(lincomb(np.concatenate([a, b]), g), total, log_n, zeta)


def deep_logup(lde, plde, qlde, g, sum1, sum2, zeta, gzeta, log_n: int, gK=None):
    """K1 = W + Wp + 8; A1 = sum_(k<W) g_k f_k + sum_(k<Wp) g_(W+k) p_k + sum_(k<8) g_(W+Wp+k) q_k, A2 = sum_(k<Wp) g_(K1+k) p_k;
    v_j = (A1 - sum1) / (x_j - zeta) + (A2 - sum2) / (x_j - gzeta). The two-point form (gK given) also opens the W columns at gzeta:
    A2 += gK sum_(k<W) g_k f_k. g: (K1 + Wp, 4)."""
    W, Wp = len(lde), len(plde)
    K1 = W + Wp + 8
    assert len(qlde) == 8 and len(g) >= K1 + Wp
    row = lincomb(lde, g[:W])
    a1 = vadd(vadd(row, lincomb(plde, g[W:W + Wp])), lincomb(qlde, g[W + Wp:K1]))
    a2 = lincomb(plde, g[K1:K1 + Wp])
    if gK is not None:
        a2 = vadd(a2, vmul(np.array(ext(gK), np.uint64)[None, :], row))
    return vadd(_quotient(a1, sum1, log_n, zeta), _quotient(a2, sum2, log_n, gzeta))


def ext_lincomb(a, b, g, second: int = 0):
    """4 columns: the coordinates of sum_(c<wa) g_c a_c + sum_(c<wb) g_(wa+c) b_c; with second != 0 four more: those of
    sum_(c<wb) g_(second+c) b_c. -> (4 or 8, len)"""
    wa, wb = len(a), len(b)
    out = lincomb(np.concatenate([a, b]), g[:wa + wb]).T
    if second:
        out = np.concatenate([out, lincomb(b, g[second:second + wb]).T])
    return out


def deep_from_combo(glde, qlde, gq, sum1, sum2, zeta, gzeta, two: bool, log_n: int):
    """v_j = (G1_j + sum_(k<8) gq_k q_k(x_j) - sum1) / (x_j - zeta) [+ (G2_j - sum2) / (x_j - gzeta) when two]; glde (8, N): the
    coordinates of G1, then of G2"""
    glde = np.asarray(glde, np.uint64)
    v = _quotient(vadd(glde[:4].T, lincomb(qlde, gq)), sum1, log_n, zeta)
    return vadd(v, _quotient(glde[4:].T, sum2, log_n, gzeta)) if two else v


# ---------------------------------------------------------------------------------------------------------- FRI
def fri_fold(v, log_size: int, shift: int, beta):
    """out[i] = (a + b) / 2 + beta (a - b) / (2 shift w^i), a = v[i], b = v[i + half], w = root(log_size); v (2 half, 4)"""
    v = vext(v)
    half = len(v) // 2
    assert len(v) == 1 << log_size
    a, b = v[:half], v[half:]
    x2inv = vinv(domain(log_size, shift)[:half] * np.uint64(2) % _p)
    return vadd(vscale(vadd(a, b), np.full(half, inv(2), np.uint64)), vmul(np.array(ext(beta), np.uint64)[None, :], vscale(vsub(a, b), x2inv)))


# ---------------------------------------------------------------------------------------------------------- scan
def scan(rowsum):
    """phi[r] = sum_(i <= r) in[i], as four columns: (H, 4) -> (4, H). A running sum of up to 2^16 words stays below 2^47."""
    return np.cumsum(vext(rowsum), axis=0, dtype=np.uint64).T % _p


# ---------------------------------------------------------------------------------------------------------- the small kernels
def quotient_split(cbr, log_h: int):
    """cbr (4, N = 2H): the unscaled DIF-iNTT of the quotient's coordinate columns. out[(4 ch + k), q] = cbr[k, 2 q + ch] *
    s^-(bitrev(q) + ch H) / 2 -> (8, H)"""
    cbr = np.asarray(cbr, np.uint64)
    H = 1 << log_h
    sinv, half = inv(SHIFT), inv(2)
    f = [np.array([pow(sinv, bitrev(q, log_h) + ch * H, P) * half % P for q in range(H)], np.uint64) for ch in (0, 1)]
    return np.concatenate([cbr[:, ch::2] * f[ch][None, :] % _p for ch in (0, 1)])


def row_layout(m, log_n: int, next_cols, step: int, selectors: bool, trace_domain: bool):
    """the columns behind an n-row matrix m (w1, n): column i = column next_cols[i] moved up by `step` rows (cyclic), then, when
    selectors, with Z_H(x) = x^H - 1 and g the generator of the TRACE domain (H rows):
      is_first_row = Z_H(x) / (x - 1),  is_last_row = Z_H(x) / (x - g^-1),  is_transition = x - g^-1
    at x_j = s w^j, w = root(log_n), H = n / 2, g = w^2 (the extended domain), or at x_j = g^j, H = n, g = root(log_n) (the trace
    domain), where the two quotients are polynomials with the values H x^(H-1) at their root (H at 1, H g at g^-1) and 0 elsewhere."""
    m = np.asarray(m, np.uint64)
    n = 1 << log_n
    out = [np.roll(m[c], -step) for c in next_cols]
    if selectors:
        w = root(log_n)
        x = domain(log_n, 1 if trace_domain else SHIFT)
        H, g = (n, w) if trace_domain else (n // 2, w * w % P)
        ginv = np.uint64(inv(g))
        if trace_domain:
            first, last = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
            first[0], last[n - 1] = H % P, H * g % P
        else:
            z = (vpow(x, H) + _p - np.uint64(1)) % _p
            first = z * vinv((x + _p - np.uint64(1)) % _p) % _p
            last = z * vinv((x + _p - ginv) % _p) % _p
        out += [first, last, (x + _p - ginv) % _p]
    return np.array(out, np.uint64).reshape(len(out), n)


def part_scatter(part, b: int, r: int, out):
    """part (n_chunks, 4, m), out (4, N) -> out with out[k, r + (i << b)] = sum_c part[c, k, i] mod p; the other rows as they were"""
    out = np.array(out, np.uint64)
    m = part.shape[2]
    out[:, r:r + (m << b):1 << b] = np.asarray(part, np.uint64).sum(axis=0) % _p
    return out


def ext_axpy(y, a, x):
    """y + a x (a None: 1)"""
    return vadd(y, x if a is None else vmul(np.array(ext(a), np.uint64)[None, :], x))


# ---------------------------------------------------------------------------------------------------------- LogUp and the quotient
# The stage in front of the kernels above (csrc/logup_kernels.hip, stark_kernels.hip, the run-time specialised kernels). Every function
# takes TABLES — blpow (max_args + 2, 4): argument j meets blpow[j + 1]; apow (folded constraints, 4) — not challenges, so a caller may
# pass tables no transcript produces. The programs are evaluated by tests/_jit_host.eval_postfix on every row at once. `it` =
# (inter, ispans, ibc) as powdr_amd.prover takes it, `starts` = the group boundaries (prover.logup_group_starts). The inverse of 0 is 0.
def _ext_rows(a, n):
    """an extension scalar on n rows"""
    return np.broadcast_to(np.array(ext(a), np.uint64), (n, 4))


def _base_rows(v, n):
    """base-field words (eval_postfix's int64, or one integer for a constant program) as n extension elements"""
    out = np.zeros((n, 4), np.uint64)
    out[:, 0] = np.broadcast_to(np.asarray(v, np.int64) % P, (n,)).astype(np.uint64)
    return out


def interaction_values(T, it, alpha, blpow):
    """per interaction: the multiplicity m_i on every row (n words) and d_i = alpha + bus_i + sum_j blpow[j + 1] a_ij (n, 4)"""
    from tests._jit_host import eval_postfix

    inter, ispans, ibc = (np.asarray(a) for a in it)
    T = np.asarray(T, np.uint64)
    n = T.shape[1]
    blpow = vext(blpow)
    span = lambda s: eval_postfix(ibc[int(ispans[s][0]):int(ispans[s][0]) + int(ispans[s][1])].tolist(), T)
    ms, ds = [], []
    for bus, n_args, s0 in inter.reshape(-1, 3).tolist():
        ms.append(_base_rows(span(s0), n)[:, 0])
        d = vadd(_ext_rows(alpha, n), _base_rows(bus, n))
        for j in range(n_args):
            d = vadd(d, vscale(blpow[j + 1][None, :], _base_rows(span(s0 + 1 + j), n)[:, 0]))
        ds.append(d)
    return ms, ds


def _group_fraction(ms, ds, i0, i1):
    """(num_g, den_g) of sum_{i0 <= i < i1} m_i / d_i: (num, den) <- (num d_i + m_i den, den d_i), as every kernel folds a group"""
    n = len(ms[i0])
    num, den = _base_rows(ms[i0].astype(np.int64), n), ds[i0]
    for i in range(i0 + 1, i1):
        num, den = vadd(vmul(num, ds[i]), vscale(den, ms[i])), vmul(den, ds[i])
    return num, den


def logup_perm(T, it, starts, alpha, blpow, vanishing=()):
    """q_g(r) = num_g(r) / den_g(r) for every group — ONE inversion per group and row, 1 / 0 = 0: a vanishing denominator d_i zeroes
    the whole group on that row —, the row sums sum_g q_g(r) and phi(r) = sum_(r' <= r) of them.
    -> (q (G, n, 4), rowsum (n, 4), phi (n, 4)). vanishing: the (interaction, row) pairs whose denominator may be 0; any other is an
    error of the CALLER's inputs (the kernels agree about 0 / 0 only where every member's multiplicity is non-zero)."""
    ms, ds = interaction_values(T, it, alpha, blpow)
    n = np.asarray(T).shape[1]
    zero = {(i, int(r)) for i, d in enumerate(ds) for r in np.flatnonzero(~d.any(axis=1))}
    assert zero <= set(vanishing), sorted(zero - set(vanishing))[:4]
    starts = [int(s) for s in starts]
    q = np.zeros((len(starts) - 1, n, 4), np.uint64)
    for g in range(len(starts) - 1):
        if starts[g + 1] > starts[g]:
            num, den = _group_fraction(ms, ds, starts[g], starts[g + 1])
            q[g] = vmul(num, vext_inv(den))
    rowsum = q.sum(axis=0) % _p
    return q, rowsum, scan(rowsum).T


def quotient_sums(T, Pm, cons, it, starts, apow, alpha=None, blpow=None):
    """the quotient's terms that read the current row alone, unscaled, on the n rows of T (W, n) and Pm (>= 4 G, n: the group columns):
    sum_c apow[c] C_c + sum_g apow[nc + g] (q_g den_g - num_g) -> (n, 4); it None: the first sum only"""
    from tests._jit_host import eval_postfix

    bc, spans = cons
    T = np.asarray(T, np.uint64)
    n = T.shape[1]
    apow = vext(apow)
    acc = np.zeros((n, 4), np.uint64)
    spans = np.asarray(spans).reshape(-1, 2).tolist()
    for c, (off, ln) in enumerate(spans):
        acc = vadd(acc, vscale(apow[c][None, :], _base_rows(eval_postfix(np.asarray(bc)[off:off + ln].tolist(), T), n)[:, 0]))
    if it is None:
        return acc
    ms, ds = interaction_values(T, it, alpha, blpow)
    Pm = np.asarray(Pm, np.uint64)
    starts = [int(s) for s in starts]
    for g in range(len(starts) - 1):
        qg = Pm[4 * g:4 * g + 4].T
        if starts[g + 1] > starts[g]:
            num, den = _group_fraction(ms, ds, starts[g], starts[g + 1])
            term = vsub(vmul(qg, den), num)
        else:
            term = qg  # an empty group: its column must vanish
        acc = vadd(acc, vmul(apow[len(spans) + g][None, :], term))
    return acc


def _boundary_and_divide(acc, phi, sumq, log_n: int, apow_tail, S):
    """(acc + apow_tail[0] is_first (phi - sumq) + apow_tail[1] is_transition (phi' - phi - sumq') + apow_tail[2] is_last (phi - S)) /
    Z_H on the N = 2^log_n rows x_j of the extended domain of a trace of H = N / 2 rows, ' = row (j + 2) mod N (the next TRACE row),
    Z_H = x^H - 1, g = root(log_n - 1): is_first = Z_H / (x - 1), is_last = Z_H / (x - 1 / g), is_transition = x - 1 / g.
    phi, sumq: (N, 4); apow_tail None: no boundary terms (a constraints-only AIR)"""
    x = domain(log_n)
    z = (vpow(x, 1 << (log_n - 1)) + _p - np.uint64(1)) % _p
    if apow_tail is not None:
        t, N = vext(apow_tail), len(x)
        ginv = np.uint64(inv(root(log_n - 1)))
        is_first = z * vinv((x + _p - np.uint64(1)) % _p) % _p
        is_last = z * vinv((x + _p - ginv) % _p) % _p
        is_trans = (x + _p - ginv) % _p
        nxt = lambda a: np.roll(a, -2, axis=0)
        acc = vadd(acc, vmul(t[0][None, :], vscale(vsub(phi, sumq), is_first)))
        acc = vadd(acc, vmul(t[1][None, :], vscale(vsub(vsub(nxt(phi), phi), nxt(sumq)), is_trans)))
        acc = vadd(acc, vmul(t[2][None, :], vscale(vsub(phi, _ext_rows(S, N)), is_last)))
    return vscale(acc, vinv(z))


def quotient(lde, plde, log_n: int, cons, it, starts, apow, alpha=None, blpow=None, S=None):
    """the quotient on the N rows of the extended domain -> (N, 4). lde (W, N); plde (>= 4 G + 4, N): the group columns, then phi —
    sum_g q_g is taken from the group columns; it None (plde, alpha, blpow, S unused): constraints only"""
    acc = quotient_sums(lde, plde, cons, it, starts, apow, alpha, blpow)
    if it is None:
        return _boundary_and_divide(acc, None, None, log_n, None, None)
    G = len(starts) - 1
    plde = np.asarray(plde, np.uint64)
    sumq = plde[:4 * G].reshape(G, 4, -1).sum(axis=0).T % _p if G else np.zeros((plde.shape[1], 4), np.uint64)
    nc = len(np.asarray(cons[1]).reshape(-1, 2))
    return _boundary_and_divide(acc, plde[4 * G:4 * G + 4].T, sumq, log_n, vext(apow)[nc + G:nc + G + 3], S)


def rowsum_combine(part):
    """part (n_chunks, 4, H) -> (H, 4): plain sums mod p"""
    return (np.asarray(part, np.uint64).sum(axis=0) % _p).T


def logup_tail(part, phi_cols, sumq_cols, log_n: int, apow_tail, S):
    """part (n_chunks, 4, N), phi_cols / sumq_cols (4, N) -> (N, 4): the boundary terms and the division on top of the summed parts"""
    return _boundary_and_divide(rowsum_combine(part), np.asarray(phi_cols, np.uint64).T, np.asarray(sumq_cols, np.uint64).T, log_n, apow_tail, S)


# ---------------------------------------------------------------------------------------------------------- the query phase
# A streamed proof answers its queries from COEFFICIENTS: c[col][k], P_col(x) = sum_k c[col][k] x^k, k < H = 2^log_h. The reference
# below starts there too, so a test of the query pass runs no transform of the code under test.
def coefficient_arrays(c, log_h: int):
    """canonical coefficients c[col][k] -> the values the device arrays hold (as Montgomery words: to_word), H c[col][bitrev(q)] at q:
    bit-reversed and H-scaled, as the inverse transform of the provers leaves them"""
    c = np.asarray(c, np.uint64).reshape(-1, 1 << log_h) % _p
    br = np.array([bitrev(q, log_h) for q in range(1 << log_h)], np.int64)
    return c[:, br] * np.uint64((1 << log_h) % P) % _p


def power_vector(x: int, n: int):
    """x^0 .. x^(n-1) for a power of two n, by doubling: the second half is the first times x^(half)"""
    pw = np.ones(1, np.uint64)
    while len(pw) < n:
        pw = np.concatenate([pw, pw * np.uint64(pow(x, len(pw), P)) % _p])
    return pw


def lde_rows(c, log_h: int, idx):
    """rows idx[q] of the extension on the 2^(log_h+1) points x_j = 31 w^j, w = root(log_h + 1): out[q][col] = sum_k c[col][k] x^k.
    Every product is reduced before the sum: 2^log_h words below p, far inside uint64."""
    c = np.asarray(c, np.uint64).reshape(-1, 1 << log_h) % _p
    w, seen, out = root(log_h + 1), {}, np.zeros((len(idx), len(c)), np.uint64)
    for q, j in enumerate(idx):
        j = int(j)
        if j not in seen:
            pw = power_vector(SHIFT * pow(w, j, P) % P, 1 << log_h)
            seen[j] = (c * pw % _p).sum(axis=1) % _p
        out[q] = seen[j]
    return out


def pow_families(rng):
    """inputs of the proof-of-work tests, (sponge state, 7 pending words) per family: random, all 0, all p - 1, the edge words"""
    from tests import _edge_values as ev

    return {"random": (rng.integers(0, P, 16, dtype=np.uint32), rng.integers(0, P, 7, dtype=np.uint32)),
            "zero": (np.zeros(16, np.uint32), np.zeros(7, np.uint32)),
            "pm1": (np.full(16, P - 1, np.uint32), np.full(7, P - 1, np.uint32)),
            "edge": (ev.EDGE[rng.integers(0, len(ev.EDGE), 16)], ev.EDGE[rng.integers(0, len(ev.EDGE), 7)])}


def gather_rows(m, idx):
    """m[col][row] -> out[q][col] = m[col][idx[q]]"""
    return np.asarray(m)[:, np.asarray(idx, np.int64)].T.copy()


def gather_records(arena, offsets, words: int):
    """out[r] = arena[offsets[r] : offsets[r] + words]"""
    arena = np.asarray(arena)
    return np.stack([arena[int(o):int(o) + words] for o in offsets])


def ext_to_cols(v):
    """len elements of 4 coordinates -> 4 columns of len"""
    return np.asarray(v).reshape(-1, 4).T.copy()


# ---------------------------------------------------------------------------------------------------------- scalar twins
# The same stages with Python integers only, row by row: what test_stage_ref_cpu.py holds the vectorised routines above against.
def lincomb_scalar(m, g):
    out = []
    for j in range(len(m[0]) if len(m) else 0):
        acc = ZERO
        for k in range(len(m)):
            acc = ext_add(acc, ext_scale(ext(g[k]), int(m[k][j])))
        out.append(acc)
    return out


def deep_scalar(a, b, g, total, zeta, log_n: int):
    num = lincomb_scalar(list(a) + list(b), g)
    x = domain(log_n)
    return [ext_mul(ext_sub(num[j], ext(total)), ext_inv(ext_sub(ext(int(x[j])), ext(zeta)))) for j in range(1 << log_n)]


def ext_dot_scalar(cols, w):
    return [functools.reduce(ext_add, (ext_scale(ext(w[q]), int(col[q])) for q in range(len(col))), ZERO) for col in cols]


def fri_fold_scalar(v, log_size: int, shift: int, beta):
    half, w = len(v) // 2, root(log_size)
    out = []
    for i in range(half):
        a, b = ext(v[i]), ext(v[i + half])
        x = shift * pow(w, i, P) % P
        out.append(ext_add(ext_scale(ext_add(a, b), inv(2)), ext_mul(ext(beta), ext_scale(ext_sub(a, b), inv(2 * x)))))
    return out


def scan_scalar(rowsum):
    acc, out = ZERO, []
    for e in rowsum:
        acc = ext_add(acc, ext(e))
        out.append(acc)
    return [[o[k] for o in out] for k in range(4)]
