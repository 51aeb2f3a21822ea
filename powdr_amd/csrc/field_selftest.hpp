// Self-test of the range-sensitive field helpers (babybear.hpp, ext.hpp) against plain 64-bit modular arithmetic, on
// random values and on the edges of the ranges their comments promise. One function for host and device: on the
// device the inline multiply-add instructions are exercised, on the host their portable fall-backs.
#pragma once
#include "ext.hpp"
#include "poseidon2.hpp"

namespace pw {

// The Poseidon2 permutation from the DEFINITION fields of Params (ext_rc, int_rc, diag) alone, on canonical Montgomery words with
// bb::add / bb::mul: the shape oracle/stark_oracle.cpp states, none of the derived tables, no signed form.
PW_HD void selftest_permute_ref(uint32_t* s, const p2::Params& P) {
    auto linear = [&]() {
        uint32_t t[16];
        for (int b = 0; b < 4; ++b) {
            const uint32_t x0 = s[4 * b], x1 = s[4 * b + 1], x2 = s[4 * b + 2], x3 = s[4 * b + 3];
            const uint32_t all = bb::add(bb::add(x0, x1), bb::add(x2, x3));
            t[4 * b] = bb::add(bb::add(all, x0), bb::double_(x1));       // 2 3 1 1
            t[4 * b + 1] = bb::add(bb::add(all, x1), bb::double_(x2));   // 1 2 3 1
            t[4 * b + 2] = bb::add(bb::add(all, x2), bb::double_(x3));   // 1 1 2 3
            t[4 * b + 3] = bb::add(bb::add(all, x3), bb::double_(x0));   // 3 1 1 2
        }
        for (int i = 0; i < 4; ++i) {
            const uint32_t col = bb::add(bb::add(t[i], t[4 + i]), bb::add(t[8 + i], t[12 + i]));
            for (int b = 0; b < 4; ++b) s[4 * b + i] = bb::add(t[4 * b + i], col);
        }
    };
    auto sbox = [](uint32_t x) { const uint32_t x2 = bb::mul(x, x), x3 = bb::mul(x2, x), x4 = bb::mul(x2, x2); return bb::mul(x3, x4); };
    linear();
#pragma unroll 1
    for (int r = 0; r < 21; ++r) {
        if (r >= 4 && r < 17) {
            s[0] = sbox(bb::add(s[0], P.int_rc[r - 4]));
            uint32_t sum = 0;
            for (int i = 0; i < 16; ++i) sum = bb::add(sum, s[i]);
            for (int i = 0; i < 16; ++i) s[i] = bb::add(sum, bb::mul(P.diag[i], s[i]));
        } else {
            const int e = r < 4 ? r : r - 13;
            for (int i = 0; i < 16; ++i) s[i] = sbox(bb::add(s[i], P.ext_rc[e][i]));
            linear();
        }
    }
}

// returns 0 or the number of the first failing check. `params`: the installed Poseidon2 table (checks 38 to 40 run the whole
// permutation under it); a null pointer is failure 40, never a silent skip.
PW_HD int field_selftest_checks(uint64_t seed, uint32_t iterations, const p2::Params* params) {
    using namespace bb;
    uint64_t s = seed ? seed : 1;
    auto rnd = [&]() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); };
    auto rp = [&]() { return (uint32_t)(rnd() % P); };
    const uint64_t edges64[] = {0, 1, P - 1, P, P + 1, 2ull * P - 1, 2ull * P, 16ull * P - 1, 75ull * P, 128ull * P - 1};
    for (uint64_t x : edges64) {
        if (x < 16ull * P && reduce_sum(x) != x % P) return 1;
        const uint32_t l = reduce_wide_loose(x);
        if (l % P != x % P || l >= (uint64_t)P + P / 32) return 2;
        if (reduce_wide(x) != x % P) return 3;
    }
    const uint32_t edges[] = {0, 1, P - 1, P, P + 1, 2 * P - 1};
    for (uint32_t a : edges)
        for (uint32_t b : edges) {
            const uint32_t r = add_2p(a, b), d = sub_2p(a, b);
            if (r >= 2 * P || r % P != (uint32_t)(((uint64_t)a + b) % P)) return 4;
            if (d >= 2 * P || d % P != (uint32_t)(((uint64_t)a + 2ull * P - b) % P)) return 5;
        }
    // signed representatives: reduction of wide sums, the S-box and the internal layer at the edges of their ranges
    auto smodp = [](int64_t v) { const int64_t r = v % (int64_t)P; return (uint32_t)(r < 0 ? r + P : r); };
    {
        // (checks 6 and 8 keep their first range, |y| < 64 p; the whole domain |y| < 128 p and the last layer's interval: 32, 33)
        const int64_t ys[] = {0, 1, -1, (int64_t)P, -(int64_t)P, 64ll * P - 1, -64ll * P + 1, 43ll * P, -43ll * P, 12345678901ll, -12345678901ll};
        for (int64_t y : ys) {
            const int32_t r = sreduce_wide_loose(y);
            if (smodp(r) != smodp(y) || r <= -(int32_t)(P / 50) || r >= (int32_t)(P + P / 50)) return 6;
            if (r > -(int32_t)P && canonical_of(r) != smodp(y)) return 6;
        }
        const int32_t hi = (int32_t)((uint64_t)P + (uint64_t)P * 45 / 1000);  // 1.045 p
        const int32_t xs[] = {0, 1, -1, (int32_t)P - 1, (int32_t)P, -(int32_t)P, hi - 1, -(hi - 1), (int32_t)(P / 2), -(int32_t)(P / 2)};
        for (int32_t x : xs) {
            uint32_t want = R_MOD_P;
            for (int k = 0; k < 7; ++k) want = mul(want, smodp(x));
            const int32_t l = p2::sbox7(x);
            if (smodp(l) != want || l <= -(int32_t)P || l >= (int32_t)P) return 7;
        }
    }
    for (uint32_t it = 0; it < 4 + iterations / 16; ++it) {
        // internal_layer with arbitrary (centred) constants: out_i = (kappa s_0 + sum_{i>=1} s_i) / R * rho / R + s_i m_i / R (+ constants)
        const int32_t top0 = (int32_t)((uint64_t)P * 97 / 100), top = (int32_t)((uint64_t)P * 92 / 100);  // |s_0| < 0.97 p, others < 0.92 p
        int32_t st[16], m[16];
        uint32_t want[16];
        for (int i = 0; i < 16; ++i) {
            const int32_t hi = i ? top : top0;
            const int32_t mag = it < 3 ? hi - 1 : (int32_t)(rnd() % (uint64_t)hi);
            st[i] = it == 0 ? mag : it == 1 ? -mag : it == 2 ? ((i & 1) ? mag : -mag) : ((rnd() & 1) ? mag : -mag);
            m[i] = it < 3 ? ((i & 2) ? (int32_t)(P / 2) : -(int32_t)(P / 2)) : centred(rp());
        }
        const int32_t kappa = it < 3 ? ((it & 1) ? (int32_t)(P / 2) : -(int32_t)(P / 2)) : centred(rp());
        const int32_t rho = it < 3 ? ((it & 2) ? (int32_t)(P / 2) : -(int32_t)(P / 2)) : centred(rp());
        const uint32_t next = it < 3 ? P - 1 : rp(), ex = it < 3 ? (P + 1) / 2 : rp();
        int64_t exit_c[16];
        for (int i = 0; i < 16; ++i) exit_c[i] = (int64_t)centred(ex) * (int64_t)R_MOD_P;
        const bool last = it & 1;
        // reference with canonical Montgomery arithmetic: x / R = mul(x, 1)
        uint32_t wide = mul(mul(smodp(st[0]), smodp(kappa)), R2_MOD_P);  // s_0 kappa (exact product, as a residue)
        for (int i = 1; i < 16; ++i) wide = add(wide, smodp(st[i]));
        const uint32_t sum = mul(wide, 1u);
        const uint32_t sum_r = mul(mul(sum, smodp(rho)), R2_MOD_P);      // sum * rho as a residue
        for (int i = 0; i < 16; ++i) {
            const uint32_t prod = mul(mul(smodp(st[i]), smodp(m[i])), R2_MOD_P);
            const uint32_t c = i ? (last ? mul(mul(smodp(centred(ex)), R_MOD_P), R2_MOD_P) : 0u) : mul(mul(smodp(centred(next)), R_MOD_P), R2_MOD_P);
            want[i] = mul(add(add(sum_r, prod), c), 1u);
        }
        if (last) p2::internal_layer<true>(st, m, kappa, rho, (int64_t)centred(next) * (int64_t)R_MOD_P, exit_c);
        else p2::internal_layer<false>(st, m, kappa, rho, (int64_t)centred(next) * (int64_t)R_MOD_P, exit_c);
        for (int i = 0; i < 16; ++i)
            if (smodp(st[i]) != want[i]) return 9;
        for (int i = 0; i < 16; ++i)
            if (st[i] <= -(int32_t)P || st[i] >= (int32_t)P) return 9;
    }
    // ---- Poseidon2's signed ranges at their edges (checks 30 and up; every figure: p2::bounds, computed by tools/poseidon2_bounds.py)
    namespace B = p2::bounds;
    const int32_t HALF = (int32_t)((P - 1) / 2);
    {   // smont on the whole of |t| < 2^63 - 2^31 p: r 2^32 == t (mod p), and r within p / 2 + 1 of t / 2^32
        auto smont_ok = [&](int64_t t) {
            const int32_t r = smont(t);
            if ((uint64_t)smodp(r) * R_MOD_P % P != smodp(t)) return false;
            const int64_t d = (int64_t)r - (t >> 32);
            return d <= (int64_t)(P / 2) + 1 && -d <= (int64_t)(P / 2) + 1;
        };
        const int64_t ts[] = {0, 1, -1, 0xffffffffll, -0xffffffffll, B::kSmontDomain - 1, -(B::kSmontDomain - 1)};
        for (int64_t t : ts)
            if (!smont_ok(t)) return 30;
        for (uint32_t it = 0; it < 16 + iterations; ++it) {
            const int64_t u = (int64_t)(rnd() % (uint64_t)B::kSmontDomain);
            if (!smont_ok((rnd() & 1) ? u : -u)) return 31;
        }
    }
    {   // sreduce_wide_loose on the whole of |y| < 128 p: congruent, inside the envelope y E / 2^39 + [0, kSreduceRound) (exclusive
        // bounds (-m - 1, m + kSreduceRound), m = floor(|y| E / 2^39)), non-negative for y >= 0
        auto sreduce_ok = [&](int64_t y) {
            const int32_t r = sreduce_wide_loose(y);
            if (smodp(r) != smodp(y)) return false;
            const uint64_t mag = (uint64_t)(y < 0 ? -y : y);
            const int64_t m = (int64_t)(((mag >> 7) * (uint64_t)B::kSreduceE + ((mag & 127) * (uint64_t)B::kSreduceE >> 7)) >> 32);  // exact floor
            if ((int64_t)r <= -m - 1 || (int64_t)r >= m + B::kSreduceRound) return false;
            return y < 0 || r >= 0;
        };
        const int64_t ys[] = {64ll * P, 64ll * P - 1, B::kLastWideLo, B::kLastWideHi - 1, B::kLastWideHi, B::kClosureWide - 1, B::kClosureWide,
                              B::kSreduceDomain - 1};
        for (int64_t y : ys)
            if (!sreduce_ok(y) || !sreduce_ok(-y)) return 32;
        // the interval the last layer really hands over: [0, 1.0207 p), so that one conditional subtraction makes the word canonical
        const int64_t last[] = {B::kLastWideLo, B::kLastWideLo + 1, 40ll * P, 60ll * P, B::kLastWideHi - 2, B::kLastWideHi - 1};
        for (int64_t y : last) {
            const int32_t r = sreduce_wide_loose(y);
            if (r < 0 || r >= B::kInputTop || reduce_2p((uint32_t)r) != smodp(y)) return 32;
        }
        for (uint32_t it = 0; it < 16 + iterations; ++it) {
            const int64_t u = (int64_t)(rnd() % (uint64_t)B::kSreduceDomain);
            if (!sreduce_ok((rnd() & 1) ? u : -u)) return 33;
            const int64_t y = B::kLastWideLo + (int64_t)(rnd() % (uint64_t)(B::kLastWideHi - B::kLastWideLo));
            const int32_t r = sreduce_wide_loose(y);
            if (r < 0 || r >= B::kInputTop || smodp(r) != smodp(y)) return 33;
        }
    }
    // external_layer, all three instantiations: every word at +-(X - 1) for the layer's input bound X (sign patterns: all +, all -,
    // alternating by word, by block, random interior values), every folded constant at +-HALF (all +, all -, the sign of its input,
    // the opposite sign, random centred values), against M4 and the column sums on canonical residues with %.
    // kind 0: constants, fed by permutation inputs; 1: constants, fed by S-box outputs; 2: no constants (before the partial rounds);
    // 3: the last layer (bias, Barrett-style reduction)
#pragma unroll 1
    for (int kind = 0; kind < 4; ++kind) {
        const int32_t X = kind == 0 ? B::kLayerInTop : kind == 3 ? B::kLastInTop : B::kSboxOutTop;
        const int n_fold = kind < 2 ? 5 : 1;
        // the last layer also at the two congruence edges of its sum, 35 v for sixteen equal words v: v = -(24 p + 1) / 35 (0.686 p) puts the
        // sum one below a multiple of p at -24 p - 1, where the result is negative unless the BIASED sum is not (every bias below 24 p
        // + 1 shows here); v = (11 p - 1) / 35 puts it at 11 p - 1, where the result is at the top of its envelope, above p
        const int32_t v_lo = (int32_t)((24ull * P + 1) / 35), v_hi = (int32_t)((11ull * P - 1) / 35);
        if (35ull * (uint64_t)v_lo % P != 1 || 35ull * (uint64_t)v_hi % P != P - 1 || v_lo >= B::kLastInTop) return 36;
        const int n_pat = kind == 3 ? 7 : 5 * n_fold;
#pragma unroll 1
        for (int pat = 0; pat < n_pat; ++pat) {
            const int sp = pat % (kind == 3 ? 7 : 5), fp = kind == 3 ? 0 : pat / 5;
            int32_t x[16];
            int64_t fold[16];
            for (int i = 0; i < 16; ++i) {
                const bool neg = sp == 1 || sp == 5 || (sp == 2 && (i & 1)) || (sp == 3 && ((i >> 2) & 1)) || (sp == 4 && (rnd() & 1));
                const int32_t mag = sp == 4 ? (int32_t)(rnd() % (uint64_t)X) : sp == 5 ? v_lo : sp == 6 ? v_hi : X - 1;
                x[i] = neg ? -mag : mag;
                const int32_t c = fp == 0 ? HALF : fp == 1 ? -HALF : fp == 2 ? (neg ? -HALF : HALF) : fp == 3 ? (neg ? HALF : -HALF) : centred(rp());
                fold[i] = kind < 2 ? (int64_t)c : 0;
            }
            uint64_t want[16];
            for (int q = 0; q < 4; ++q) {
                const uint64_t x0 = smodp(x[4 * q]), x1 = smodp(x[4 * q + 1]), x2 = smodp(x[4 * q + 2]), x3 = smodp(x[4 * q + 3]);
                const uint64_t a = smodp(fold[4 * q]), b = smodp(fold[4 * q + 1]), d1 = smodp(fold[4 * q + 2]), d3 = smodp(fold[4 * q + 3]);
                want[4 * q] = (2 * x0 + 3 * x1 + x2 + x3 + 2 * a + b) % P;
                want[4 * q + 1] = (x0 + 2 * x1 + 3 * x2 + x3 + a + b + d1) % P;
                want[4 * q + 2] = (x0 + x1 + 2 * x2 + 3 * x3 + a + 2 * b) % P;
                want[4 * q + 3] = (3 * x0 + x1 + x2 + 2 * x3 + a + b + d3) % P;
            }
            for (int i = 0; i < 4; ++i) {
                const uint64_t col = want[i] + want[4 + i] + want[8 + i] + want[12 + i];
                for (int q = 0; q < 4; ++q) want[4 * q + i] = (want[4 * q + i] + col) % P;
            }
            if (kind < 2) p2::external_layer<true, false>(x, fold);
            else if (kind == 2) p2::external_layer<false, false>(x, nullptr);
            else p2::external_layer<false, true>(x, nullptr);
            for (int i = 0; i < 16; ++i) {
                if (kind == 3) {  // as it is, in [0, 1.0207 p)
                    if (smodp(x[i]) != want[i] || x[i] < 0 || x[i] >= B::kInputTop) return 36;
                } else {          // times R^-1, below 0.5000 p in magnitude
                    if ((uint64_t)smodp(x[i]) * R_MOD_P % P != want[i]) return kind == 2 ? 35 : 34;
                    if (x[i] >= B::kExtOutTop || x[i] <= -B::kExtOutTop) return 37;
                }
            }
        }
    }
    // the whole permutation under the installed table against selftest_permute_ref: chains of three permutations between which the
    // first k words are overwritten with canonical words, k = 8 and 3 (leaf_hash_kernel's full and short last chunk), so that
    // permute<true> carries non-canonical words into the next one; every intermediate state is also given to permute<false>.
    // Initial states: canonical edges (0, p - 1, (p -+ 1) / 2, mixed), the non-canonical edges of [0, 1.0207 p) (p, p + 1, the top,
    // mixed), random canonical and random non-canonical ones.
    if (!params) return 40;
    {
        const uint32_t top = (uint32_t)B::kInputTop - 1;
        const uint32_t mixed[8] = {0u, P - 1, (P - 1) / 2, (P + 1) / 2, P, P + 1, top, 1u};
        const uint32_t n_cases = 2 * (10 + iterations / 64);
#pragma unroll 1
        for (uint32_t c = 0; c < n_cases; ++c) {
            const uint32_t init = c >> 1;
            const int k = (c & 1) ? 3 : 8;
            uint32_t st[16], ref[16], one[16];
            for (int i = 0; i < 16; ++i) {
                st[i] = init == 0 ? 0u : init == 1 ? P - 1 : init == 2 ? (P - 1) / 2 : init == 3 ? (P + 1) / 2 : init == 4 ? mixed[i & 3]
                      : init == 5 ? P : init == 6 ? P + 1 : init == 7 ? top : init == 8 ? mixed[(i * 5 + 4) & 7]
                      : (init & 1) ? rp() : (uint32_t)(rnd() % (uint64_t)B::kInputTop);
                ref[i] = st[i] % P;
            }
#pragma unroll 1
            for (int step = 0; step < 3; ++step) {
                if (step)
                    for (int i = 0; i < k; ++i) st[i] = ref[i] = init < 9 ? mixed[(i + step + init) & 3] : rp();
                for (int i = 0; i < 16; ++i) one[i] = st[i];
                p2::permute<false>(one, *params);
                p2::permute<true>(st, *params);
                selftest_permute_ref(ref, *params);
                for (int i = 0; i < 16; ++i) {
                    if (one[i] != ref[i]) return 38;
                    if (st[i] >= (uint32_t)B::kInputTop || st[i] % P != ref[i]) return 39;
                }
            }
            for (int i = 0; i < 16; ++i)
                if (reduce_2p(st[i]) != ref[i]) return 39;
        }
    }
    for (uint32_t it = 0; it < iterations; ++it) {
        const uint32_t a = rp(), b = rp(), c = rp(), d = rp();
        {
            const int32_t x = (int32_t)((int64_t)(rnd() % (2ull * P + P / 11)) - (int64_t)(P + P / 22));  // (-1.045 p, 1.045 p); in 64 bits: UBSan, round 6
            uint32_t want = R_MOD_P;
            for (int k = 0; k < 7; ++k) want = mul(want, smodp(x));
            if (smodp(p2::sbox7(x)) != want) return 8;
            const int64_t y = (int64_t)(rnd() % (128ull * P)) - 64ll * P;
            if (smodp(sreduce_wide_loose(y)) != smodp(y)) return 8;
        }
        // Montgomery products against the definition a*b*R^-1
        const uint32_t ab = mul(a, b);
        if (ab >= P || (uint64_t)ab * R_MOD_P % P != (uint64_t)a * b % P) return 10;
        const uint32_t m2 = mul2(a, b, c, d);
        if (m2 != add(ab, mul(c, d))) return 11;
        const uint32_t la = (uint32_t)(rnd() % (2ull * P));  // a lazy operand
        const uint32_t ml = mul_lazy(la, b);
        if (ml >= 2 * P || ml % P != mul(la % P, b)) return 12;
        if (add_2p(la, (uint32_t)(rnd() % (2ull * P))) >= 2 * P) return 13;
        const uint64_t w = rnd() % (128ull * P);
        if (reduce_wide(w) != w % P) return 14;
        const uint32_t loose = reduce_wide_loose(w);
        if (loose % P != w % P || loose >= (uint64_t)P + P / 32) return 15;
        const uint64_t w16 = rnd() % (16ull * P);
        if (reduce_sum(w16) != w16 % P) return 16;
        if (wide_add(w16, a) != w16 + a || wide_fma(w16, a, 3) != w16 + 3ull * a || wide_mul(a, 4) != 4ull * a) return 17;
        // extension field: (x*y)*z == x*(y*z), x * x^-1 == 1, wide accumulation == sum of scalings
        const Ext x{{rp(), rp(), rp(), rp()}}, y{{rp(), rp(), rp(), rp()}}, z{{rp(), rp(), rp(), rp()}};
        if (!ext_eq(ext_mul(ext_mul(x, y), z), ext_mul(x, ext_mul(y, z)))) return 20;
        if (!ext_eq(ext_mul(x, ext_add(y, z)), ext_add(ext_mul(x, y), ext_mul(x, z)))) return 21;
        if ((x.c[0] | x.c[1] | x.c[2] | x.c[3]) && !ext_eq(ext_mul(x, ext_inv(x)), ext_one())) return 22;
        ExtWideAcc acc;
        Ext want = ext_zero();
        for (int k = 0; k < 37; ++k) {
            const Ext e{{rp(), rp(), rp(), rp()}};
            const uint32_t v = rp();
            acc.fma(e, v);
            want = ext_add(want, ext_scale(e, v));
        }
        if (!ext_eq(acc.result(), want)) return 23;
        ExtProductAcc pacc;
        Ext pwant = ext_zero();
        for (int k = 0; k < 29; ++k) {
            const bool edge = k < 2;  // all coordinates p - 1: the largest raw sums
            const Ext e{{edge ? P - 1 : rp(), edge ? P - 1 : rp(), edge ? P - 1 : rp(), edge ? P - 1 : rp()}};
            const Ext f{{edge ? P - 1 : rp(), edge ? P - 1 : rp(), edge ? P - 1 : rp(), edge ? P - 1 : rp()}};
            pacc.fma(e, f);
            pwant = ext_add(pwant, ext_mul(e, f));
            const uint32_t v = k == 2 ? P - 1 : rp();
            pacc.fma_base(f, v);
            pwant = ext_add(pwant, ext_scale(f, v));
        }
        if (!ext_eq(pacc.result(), pwant)) return 24;
        // centred signed accumulation (ExtCentredAcc): four terms between folds, coordinates at the edges of the centred range
        // (both neighbours of p / 2, 0, p - 1) in the first rounds — the largest magnitudes the fold's domain has to take
        ExtCentredAcc cacc, cacc_u;
        Ext cwant = ext_zero();
        const uint32_t half_lo = (P - 1) / 2, half_hi = (P + 1) / 2;
        for (int k = 0; k < 43; ++k) {
            const uint32_t ev = k < 8 ? ((k & 1) ? half_lo : half_hi) : rp();
            const Ext e{{k < 8 ? ev : rp(), k < 8 ? ev : rp(), k < 8 ? (P - 1) : rp(), k < 8 ? 0u : rp()}};
            const uint32_t v = k < 8 ? ((k & 2) ? half_hi : half_lo) : rp();
            int32_t ec[4];
            ext_centred(e, ec);
            cacc.fma(ec, centred(v));
            cacc_u.fma_uniform(ec, centred(v));
            cwant = ext_add(cwant, ext_scale(e, v));
            if ((k & 3) == 3) { cacc.fold(); cacc_u.fold(); }
        }
        if (!ext_eq(cacc.result(), cwant) || !ext_eq(cacc_u.result(), cwant)) return 25;
    }
    return 0;
}

}  // namespace pw
