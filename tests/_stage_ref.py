"""A plain reference of the opening, DEEP, FRI, scan and layout stages (csrc/stark_kernels.hip, logup_kernels.hip, stream_kernels.hip),
one function per stage, each stating the formula of the kernel's comment. Pure Python and numpy, no library call; importable without a
GPU. Everything here is a CANONICAL value; the prime, the roots of unity and the coset shift are the oracle's. The extension is
E = F[X] / (X^4 - 11), an element = 4 coordinates, lowest degree first.

Two layers. Scalars (a challenge, an opened sum, one weight) are tuples of 4 Python integers: ext_add .. ext_pow. Whole vectors are
numpy uint64 arrays with a last axis of 4 (v*): every product of two words below p is below 2^62 and is reduced at once, a sum of 2^14
reduced words is below 2^45, so uint64 never wraps (the longest sums here: 16384 rows in ext_dot, 65536 in the scan — below 2^47).
tests/test_stage_ref_cpu.py holds the scalar layer against the oracle's field and against polynomial identities, and every v* routine
against its scalar twin."""
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
