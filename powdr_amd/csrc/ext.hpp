// Degree-4 extension E = F[X]/(X^4 - 11) of BabyBear on Montgomery words, for
// device kernels and the host transcript. Challenges (alpha, zeta, gamma, beta)
// and everything derived from them live in E; trace data stays in F.
#pragma once
#include "babybear.hpp"

namespace bb {

struct Ext {
    uint32_t c[4];
};

// 11 in Montgomery form: 11 * 2^32 mod p
PW_HD uint32_t w11() { return 939524073u; }  // 0x37ffffe9

PW_HD Ext ext_zero() { return {{0u, 0u, 0u, 0u}}; }
PW_HD Ext ext_one() { return {{R_MOD_P, 0u, 0u, 0u}}; }
PW_HD Ext ext_from_base(uint32_t a) { return {{a, 0u, 0u, 0u}}; }
PW_HD Ext ext_add(const Ext& a, const Ext& b) {
    return {{add(a.c[0], b.c[0]), add(a.c[1], b.c[1]), add(a.c[2], b.c[2]), add(a.c[3], b.c[3])}};
}
PW_HD Ext ext_sub(const Ext& a, const Ext& b) {
    return {{sub(a.c[0], b.c[0]), sub(a.c[1], b.c[1]), sub(a.c[2], b.c[2]), sub(a.c[3], b.c[3])}};
}
PW_HD Ext ext_neg(const Ext& a) { return {{neg(a.c[0]), neg(a.c[1]), neg(a.c[2]), neg(a.c[3])}}; }
PW_HD Ext ext_scale(const Ext& a, uint32_t k) {
    return {{mul(a.c[0], k), mul(a.c[1], k), mul(a.c[2], k), mul(a.c[3], k)}};
}
PW_HD bool ext_eq(const Ext& a, const Ext& b) {
    return a.c[0] == b.c[0] && a.c[1] == b.c[1] && a.c[2] == b.c[2] && a.c[3] == b.c[3];
}

// Products are reduced in pairs (bb::mul2: a*b + c*d with one Montgomery reduction), which halves the reductions and
// saves a modular addition per pair: 75 instructions instead of 131 for the schoolbook form.
PW_HD Ext ext_mul(const Ext& a, const Ext& b) {
    const uint32_t W = w11();
    // the parts that get multiplied by 11
    const uint32_t h0 = add(mul2(a.c[1], b.c[3], a.c[2], b.c[2]), mul(a.c[3], b.c[1]));
    const uint32_t h1 = mul2(a.c[2], b.c[3], a.c[3], b.c[2]);
    const uint32_t h2 = mul(a.c[3], b.c[3]);
    Ext r;
    r.c[0] = mul2(a.c[0], b.c[0], W, h0);
    r.c[1] = add(mul2(a.c[0], b.c[1], a.c[1], b.c[0]), mul(W, h1));
    r.c[2] = add(mul2(a.c[0], b.c[2], a.c[1], b.c[1]), mul2(a.c[2], b.c[0], W, h2));
    r.c[3] = add(mul2(a.c[0], b.c[3], a.c[1], b.c[2]), mul2(a.c[2], b.c[1], a.c[3], b.c[0]));
    return r;
}
PW_HD Ext ext_sqr(const Ext& a) { return ext_mul(a, a); }

// sum_k e_k * x_k with e_k in E, x_k in F, reduced once at the end: per term and coordinate one 32x32+64-bit
// multiply-add into a 96-bit accumulator (plus the carry) instead of a Montgomery product and a modular addition
// (8 instructions). The raw products of Montgomery words sum to (sum e x) R^2, so one division by R at the end
// returns the Montgomery form of the sum. Exact for up to 2^32 terms.
struct ExtWideAcc {
    uint64_t lo[4];
    uint32_t hi[4];
    PW_HD ExtWideAcc() : lo{0, 0, 0, 0}, hi{0, 0, 0, 0} {}
    PW_HD void fma(const Ext& e, uint32_t x) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t s = lo[k] + (uint64_t)e.c[k] * x;
            hi[k] += s < lo[k] ? 1u : 0u;
            lo[k] = s;
        }
    }
    PW_HD Ext result() const {
        Ext r;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            // hi 2^64 + lo (mod p), 2^64 = R^2
            const uint64_t t = (uint64_t)(hi[k] % P) * R2_MOD_P + lo[k] % P;
            r.c[k] = mul((uint32_t)(t % P), 1u);  // * R^-1
        }
        return r;
    }
};

// The same sums with CENTRED operands in signed 64-bit accumulators (round 3): e_k given as centred representatives (|e| <= p/2,
// the wave-uniform ones straight from a table the host centred), x_k centred on the fly; a product is below p^2 / 4, so FOUR terms
// (p^2) fit an int64 (2.2756 p^2; bounds::kCentredTermsPerFold) on top of what an earlier fold left (<= 0.1422 p^2), and every
// fourth term `fold` brings the accumulators back: bb::sfold, the same residue, |.| <= 0.1422 p^2. Per term and
// coordinate 1 multiply-add + 1/2 instruction of folding + a share of the centring, against a multiply-add and a carry chain (3-4).
struct ExtCentredAcc {
    int64_t a[4];
    PW_HD ExtCentredAcc() : a{0, 0, 0, 0} {}
    // e: centred coordinates, x: centred value; at most four calls between two folds
    PW_HD void fma(const int32_t (&e)[4], int32_t x) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
            int64_t out;
            asm("v_mad_i64_i32 %0, vcc, %1, %2, %3" : "=v"(out) : "v"(e[k]), "v"(x), "v"(a[k]) : "vcc");
            a[k] = out;
#else
            a[k] += (int64_t)e[k] * x;
#endif
        }
    }
    PW_HD void fma_uniform(const int32_t (&e)[4], int32_t x) {  // e wave-uniform (scalar registers)
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = swide_mad_uniform(a[k], x, e[k]);
    }
    PW_HD void fold() {
#pragma unroll
        for (int k = 0; k < 4; ++k) a[k] = sfold(a[k]);
    }
    // the raw products of Montgomery words carry R^2: one signed reduction returns the Montgomery form of the sum
    PW_HD Ext result() {
        fold();  // |a| <= 0.14 p^2: the reduction below lands in (-0.57 p, 0.57 p)
        Ext r;
#pragma unroll
        for (int k = 0; k < 4; ++k) r.c[k] = canonical_of(smont(a[k]));
        return r;
    }
};
PW_HD void ext_centred(const Ext& e, int32_t (&out)[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = centred(e.c[k]);
}

// sum_k a_k * c_k with a_k, c_k in E, reduced once at the end: the seven coefficients of the product polynomial
// (before X^4 = 11) are sums of at most four raw 64-bit products (4 p^2 < 2^64) and go into 96-bit accumulators — 16
// multiply-adds + 7 carries per term where ext_mul + ext_add take 87 instructions. Exact for up to 2^32 terms.
struct ExtProductAcc {
    uint64_t lo[7];
    uint32_t hi[7];
    PW_HD ExtProductAcc() : lo{0, 0, 0, 0, 0, 0, 0}, hi{0, 0, 0, 0, 0, 0, 0} {}
    PW_HD void add_raw(int k, uint64_t e) {
        const uint64_t s = lo[k] + e;
        hi[k] += s < e ? 1u : 0u;
        lo[k] = s;
    }
    PW_HD void fma(const Ext& a, const Ext& c) {
        add_raw(0, (uint64_t)a.c[0] * c.c[0]);
        add_raw(1, (uint64_t)a.c[0] * c.c[1] + (uint64_t)a.c[1] * c.c[0]);
        add_raw(2, (uint64_t)a.c[0] * c.c[2] + (uint64_t)a.c[1] * c.c[1] + (uint64_t)a.c[2] * c.c[0]);
        add_raw(3, ((uint64_t)a.c[0] * c.c[3] + (uint64_t)a.c[1] * c.c[2]) + ((uint64_t)a.c[2] * c.c[1] + (uint64_t)a.c[3] * c.c[0]));
        add_raw(4, (uint64_t)a.c[1] * c.c[3] + (uint64_t)a.c[2] * c.c[2] + (uint64_t)a.c[3] * c.c[1]);
        add_raw(5, (uint64_t)a.c[2] * c.c[3] + (uint64_t)a.c[3] * c.c[2]);
        add_raw(6, (uint64_t)a.c[3] * c.c[3]);
    }
    PW_HD void fma_base(const Ext& a, uint32_t x) {  // a * (x, 0, 0, 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) add_raw(k, (uint64_t)a.c[k] * x);
    }
    PW_HD Ext result() const {
        uint32_t r[7];
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            // hi 2^64 + lo (mod p), 2^64 = R^2; the raw products carry R^2, one division by R returns Montgomery form
            const uint64_t t = (uint64_t)(hi[k] % P) * R2_MOD_P + lo[k] % P;
            r[k] = mul((uint32_t)(t % P), 1u);
        }
        const uint32_t W = w11();
        return {{add(r[0], mul(W, r[4])), add(r[1], mul(W, r[5])), add(r[2], mul(W, r[6])), r[3]}};
    }
};

// ---- the signed form --------------------------------------------------------------------------------------------------------------
// The same field on SIGNED representatives of Montgomery words (int32 coordinates), for code that is bound by its vector
// instructions (the LogUp kernels, jit_device.hpp). Sums of raw products live in int64 registers and are reduced by bb::smont (sums of
// one or two products) or bb::smont_any (everything longer: the fold makes the reduction's domain all of int64), so no operation
// needs a conditional subtraction and nothing is ever re-centred. Classes of representatives, all as INCLUSIVE magnitudes:
//   centred  |x| <= kHalf          canonical words centred on load, wave-uniform challenges
//   S        |x| <= kSmontAnyMax   every output of smont_any (0.5667 p); contains the centred ones
//   W        |x| <= kWideMax       sext_scale2's outputs (0.7656 p): good as the FIRST operand of a product, for stores and addends
// tools/ext_signed_bounds.py computes every figure below from these three and reads this block back.
namespace bounds {
constexpr int32_t kHalf = 1006632960;                   // (p - 1) / 2
constexpr int32_t kPre11Max = 1256194042;               // |11 x| for x in S (SExtB::w: smont of a one-term product)
constexpr int32_t kWideMax = 1541406720;                // class W
constexpr int32_t kScaleMax = 1274019840;               // sext_scale: S times a centred word
constexpr int64_t kMulAddendMax = 1148417904979476480ll;  // the fifth term of sext_mul_add_scaled / sext_mul_sub / sext_mul_sub_base
constexpr int64_t kMulSumMax = 8893641656830525440ll;   // a coordinate sum of a product W x S plus that addend: 2.194 p^2 of 2.2756 p^2
constexpr int64_t kMulSub2SumMax = 7354941117290250240ll;  // sext_mul_sub_scaled2: a centred first operand, two scaled class-S words: 1.814 p^2
constexpr int64_t kNormSumMax = 2734670129387274240ll;  // d0^2 - 11 d1^2 before its plain reduction
constexpr int32_t kNormMax = 1643347966;                // |n| of SExtInvPrep
constexpr int32_t kChainMax = 1643347966;               // where products of two chain words close under smont: the inversion chain
constexpr int32_t kInvEMax = 1443147263;                // |d0 / n|, |d1 / n| in sext_inv_finish
constexpr int32_t kInvE11Max = 1322321416;              // and 11 times that
constexpr int64_t kDenTerm = 2026619832316723200ll;     // a canonical argument times a centred challenge coordinate
constexpr int32_t kDenTermsPerFold = 4;                 // how many of them fit on top of a folded sum (pwj::DenominatorAcc)
constexpr int32_t kCentredTermsPerFold = 8;             // the same for two centred factors (ExtCentredAcc; its callers fold every fourth)
constexpr int64_t kAccTerm = 1148417904979476480ll;     // SExtProductAcc: a centred challenge coordinate times a class-S word
constexpr int32_t kAccPeriod0 = 7;                      // terms between folds of coefficients 0 and 6 (one product per term),
constexpr int32_t kAccPeriod1 = 3;                      // 1 and 5 (two),
constexpr int32_t kAccPeriod2 = 2;                      // 2 and 4 (three),
constexpr int32_t kAccPeriod3 = 1;                      // 3 (four)
constexpr int32_t kAccOutMax = 1390411770;              // SExtProductAcc::result before canonical_of_centred
}  // namespace bounds
static_assert(bounds::kHalf == (int32_t)((P - 1) / 2) && bounds::kHalf <= bounds::kSmontAnyMax, "centred words are in S");
static_assert(bounds::kWideMax < (int32_t)P && bounds::kScaleMax < (int32_t)P && bounds::kAccOutMax < (int32_t)P, "canonical_of_centred takes (-p, p)");
static_assert(4 * (int64_t)bounds::kWideMax * bounds::kPre11Max + bounds::kMulAddendMax == bounds::kMulSumMax, "a product's coordinate sums (an int64 literal: they fit)");
static_assert((int64_t)bounds::kChainMax * bounds::kChainMax <= bounds::kSmontDomain && bounds::kNormSumMax <= bounds::kSmontDomain, "the inversion chain stays with smont");
static_assert((0x7fffffffffffffffll - bounds::kSfoldMax) / bounds::kDenTerm == bounds::kDenTermsPerFold, "denominator terms between folds");
static_assert((0x7fffffffffffffffll - bounds::kSfoldMax) / (4 * bounds::kAccTerm) == bounds::kAccPeriod3 &&
              (0x7fffffffffffffffll - bounds::kSfoldMax) / (3 * bounds::kAccTerm) == bounds::kAccPeriod2 &&
              (0x7fffffffffffffffll - bounds::kSfoldMax) / (2 * bounds::kAccTerm) == bounds::kAccPeriod1 &&
              (0x7fffffffffffffffll - bounds::kSfoldMax) / bounds::kAccTerm == bounds::kAccPeriod0, "product accumulator terms between folds");

struct SExt {
    int32_t c[4];
};
constexpr int32_t kW11 = 939524073;  // 11 in Montgomery form (w11()): below p / 2, so centred as it stands

PW_HD SExt sext_zero() { return {{0, 0, 0, 0}}; }
PW_HD SExt sext_one() { return {{(int32_t)R_MOD_P, 0, 0, 0}}; }
// canonical words -> centred; any representative in (-p, p) -> canonical words
PW_HD SExt sext_centred(const Ext& a) { return {{centred(a.c[0]), centred(a.c[1]), centred(a.c[2]), centred(a.c[3])}}; }
PW_HD Ext sext_canonical(const SExt& a) {
    return {{canonical_of_centred(a.c[0]), canonical_of_centred(a.c[1]), canonical_of_centred(a.c[2]), canonical_of_centred(a.c[3])}};
}
// Sums and differences only add the magnitudes: S +- S is up to 1.1334 p, beyond an int32 (2^31 = 1.0667 p), so they are defined for
// centred operands (|out| <= p - 1: good for canonical_of_centred, NOT an operand of a product). The kernels never need them: what
// would be added is made a further term of a product's coordinate sums instead (sext_mul_add_scaled, sext_mul_sub).
PW_HD SExt sext_add(const SExt& a, const SExt& b) { return {{a.c[0] + b.c[0], a.c[1] + b.c[1], a.c[2] + b.c[2], a.c[3] + b.c[3]}}; }
PW_HD SExt sext_sub(const SExt& a, const SExt& b) { return {{a.c[0] - b.c[0], a.c[1] - b.c[1], a.c[2] - b.c[2], a.c[3] - b.c[3]}}; }

// The second operand of a product with the factor 11 of X^4 = 11 folded in: w[k] = 11 c[k + 1] (one plain reduction each, made once
// however many products the operand enters). c in S, |w| <= kPre11Max.
struct SExtB {
    int32_t c[4];
    int32_t w[3];
};
PW_HD SExtB sext_prepare(const SExt& b) {
    return {{b.c[0], b.c[1], b.c[2], b.c[3]}, {smont(smul_uniform(b.c[1], kW11)), smont(smul_uniform(b.c[2], kW11)), smont(smul_uniform(b.c[3], kW11))}};
}
// the four coordinate sums of a b (raw: they carry R^2) on top of the addends t[]
PW_HD void sext_mul_raw(const SExt& a, const SExtB& b, int64_t (&t)[4]) {
    t[0] = smad(smad(smad(smad(t[0], a.c[0], b.c[0]), a.c[1], b.w[2]), a.c[2], b.w[1]), a.c[3], b.w[0]);
    t[1] = smad(smad(smad(smad(t[1], a.c[0], b.c[1]), a.c[1], b.c[0]), a.c[2], b.w[2]), a.c[3], b.w[1]);
    t[2] = smad(smad(smad(smad(t[2], a.c[0], b.c[2]), a.c[1], b.c[1]), a.c[2], b.c[0]), a.c[3], b.w[2]);
    t[3] = smad(smad(smad(smad(t[3], a.c[0], b.c[3]), a.c[1], b.c[2]), a.c[2], b.c[1]), a.c[3], b.c[0]);
}
PW_HD SExt sext_reduce(const int64_t (&t)[4]) { return {{smont_any(t[0]), smont_any(t[1]), smont_any(t[2]), smont_any(t[3])}}; }
// a b: a in W, b in S -> S. 16 multiply-adds + four fold reductions (+ 9 for the prepared operand): 41 instructions against ext_mul's 75.
PW_HD SExt sext_mul(const SExt& a, const SExtB& b) {
    int64_t t[4] = {smul(a.c[0], b.c[0]), smul(a.c[0], b.c[1]), smul(a.c[0], b.c[2]), smul(a.c[0], b.c[3])};
    t[0] = smad(smad(smad(t[0], a.c[1], b.w[2]), a.c[2], b.w[1]), a.c[3], b.w[0]);
    t[1] = smad(smad(smad(t[1], a.c[1], b.c[0]), a.c[2], b.w[2]), a.c[3], b.w[1]);
    t[2] = smad(smad(smad(t[2], a.c[1], b.c[1]), a.c[2], b.c[0]), a.c[3], b.w[2]);
    t[3] = smad(smad(smad(t[3], a.c[1], b.c[2]), a.c[2], b.c[1]), a.c[3], b.c[0]);
    return sext_reduce(t);
}
PW_HD SExt sext_mul(const SExt& a, const SExt& b) { return sext_mul(a, sext_prepare(b)); }
// a b + c x for a centred base word x (c in S): the scaled term is a fifth product of every coordinate sum (it carries R^2 like them)
PW_HD SExt sext_mul_add_scaled(const SExt& a, const SExtB& b, const SExt& c, int32_t x) {
    int64_t t[4] = {smul(c.c[0], x), smul(c.c[1], x), smul(c.c[2], x), smul(c.c[3], x)};
    sext_mul_raw(a, b, t);
    return sext_reduce(t);
}
// a b - c (c in W): c carries R where the sums carry R^2, so it enters as c (-kappa)
PW_HD SExt sext_mul_sub(const SExt& a, const SExtB& b, const SExt& c) {
    const int32_t nk = -(int32_t)R_MOD_P;
    int64_t t[4] = {smul_uniform(c.c[0], nk), smul_uniform(c.c[1], nk), smul_uniform(c.c[2], nk), smul_uniform(c.c[3], nk)};
    sext_mul_raw(a, b, t);
    return sext_reduce(t);
}
// a b - (c x + d y) for a CENTRED a (|a| <= kHalf) and centred base words x, y (c, d in S): the term q d0 d1 - (m0 d1 + m1 d0) of a
// two-member group in one set of coordinate sums (<= kMulSub2SumMax) — the scaled words carry R^2 like the products, so the numerator
// needs no reduction of its own
PW_HD SExt sext_mul_sub_scaled2(const SExt& a, const SExtB& b, const SExt& c, int32_t x, const SExt& d, int32_t y) {
    const int32_t nx = -x, ny = -y;
    int64_t t[4] = {smad(smul(c.c[0], nx), d.c[0], ny), smad(smul(c.c[1], nx), d.c[1], ny), smad(smul(c.c[2], nx), d.c[2], ny), smad(smul(c.c[3], nx), d.c[3], ny)};
    sext_mul_raw(a, b, t);
    return sext_reduce(t);
}
// a b - (x, 0, 0, 0) for a centred base word x
PW_HD SExt sext_mul_sub_base(const SExt& a, const SExtB& b, int32_t x) {
    int64_t t[4] = {smul_uniform(x, -(int32_t)R_MOD_P), 0, 0, 0};
    sext_mul_raw(a, b, t);
    return sext_reduce(t);
}
// a^2 for a in S: ten products, the doubled ones added twice as 64-bit values
PW_HD SExt sext_sqr(const SExt& a) {
    const int32_t w2 = smont(smul_uniform(a.c[2], kW11)), w3 = smont(smul_uniform(a.c[3], kW11));
    const int64_t x13 = smul(a.c[1], w3), x01 = smad(smul(a.c[0], a.c[1]), a.c[2], w3), x02 = smul(a.c[0], a.c[2]),
                  x03 = smad(smul(a.c[0], a.c[3]), a.c[1], a.c[2]);
    const int64_t t[4] = {smad(smad(x13 + x13, a.c[0], a.c[0]), a.c[2], w2), x01 + x01, smad(smad(x02 + x02, a.c[1], a.c[1]), a.c[3], w3), x03 + x03};
    return sext_reduce(t);
}
// a x for a centred base word x: a in S -> |out| <= kScaleMax (stores and addends; through smont_any it would be S)
PW_HD SExt sext_scale(const SExt& a, int32_t x) {
    return {{smont(smul(a.c[0], x)), smont(smul(a.c[1], x)), smont(smul(a.c[2], x)), smont(smul(a.c[3], x))}};
}
// a x + b y for centred base words x, y: two products per plain reduction; a, b in S -> W
PW_HD SExt sext_scale2(const SExt& a, int32_t x, const SExt& b, int32_t y) {
    return {{smont(smad(smul(a.c[0], x), b.c[0], y)), smont(smad(smul(a.c[1], x), b.c[1], y)), smont(smad(smul(a.c[2], x), b.c[2], y)),
             smont(smad(smul(a.c[3], x), b.c[3], y))}};
}

// The inverse (as ext_inv below: norm to the quadratic subfield, then to the base field), split around its one base-field inversion.
// a in S. d0 = a0^2 + 11 a2^2 - 22 a1 a3 and d1 = 2 a0 a2 - a1^2 - 11 a3^2 are four-product sums (-> S); the norm n = d0^2 - 11 d1^2 is a
// two-product sum inside smont's domain (|n| <= kNormMax). The caller inverts n (a chain of plain products, closed at kChainMax).
struct SExtInvPrep {
    int32_t d0, d1, n;
};
PW_HD SExtInvPrep sext_inv_prepare(const SExt& a) {
    const int32_t w2 = smont(smul_uniform(a.c[2], kW11)), nw3 = smont(smul_uniform(a.c[3], -kW11)), na1 = -a.c[1];
    const int64_t x13 = smul(a.c[1], nw3), x02 = smul(a.c[0], a.c[2]);
    SExtInvPrep r;
    r.d0 = smont_any(smad(smad(x13 + x13, a.c[0], a.c[0]), a.c[2], w2));
    r.d1 = smont_any(smad(smad(x02 + x02, na1, a.c[1]), a.c[3], nw3));
    r.n = smont(smad(smul(r.d0, r.d0), r.d1, smont(smul_uniform(r.d1, -kW11))));
    return r;
}
// n_inv: a chain word (|.| <= kChainMax) -> a^-1 in S
PW_HD SExt sext_inv_finish(const SExt& a, const SExtInvPrep& p, int32_t n_inv) {
    const int32_t e0 = smont(smul(p.d0, n_inv)), ne1 = smont(smul(p.d1, n_inv));  // E = (d0 - d1 Y) / n
    const int32_t ne0 = -e0, e1 = -ne1, e1w = smont(smul_uniform(e1, kW11)), ne1w = -e1w;
    // (A0 - A1 X) E:  A0 E = (a0 e0 + 11 a2 e1, a0 e1 + a2 e0), -A1 E likewise
    return {{smont_any(smad(smul(a.c[0], e0), a.c[2], e1w)), smont_any(smad(smul(a.c[1], ne0), a.c[3], ne1w)),
             smont_any(smad(smul(a.c[0], e1), a.c[2], e0)), smont_any(smad(smul(a.c[1], ne1), a.c[3], ne0))}};
}
PW_HD int32_t smulm(int32_t x, int32_t y) { return smont(smul(x, y)); }
// x^(p-2) on chain words (bb::inv's addition chain, three instructions a product); 0 -> 0
PW_HD int32_t sinv(int32_t a) {
    const int32_t x3 = smulm(smulm(a, a), a), x7 = smulm(smulm(x3, x3), a);
    int32_t o6 = x7;
    for (int i = 0; i < 3; ++i) o6 = smulm(o6, o6);
    o6 = smulm(o6, x7);
    int32_t o12 = o6;
    for (int i = 0; i < 6; ++i) o12 = smulm(o12, o12);
    o12 = smulm(o12, o6);
    int32_t o24 = o12;
    for (int i = 0; i < 12; ++i) o24 = smulm(o24, o24);
    o24 = smulm(o24, o12);
    int32_t o27 = o24;
    for (int i = 0; i < 3; ++i) o27 = smulm(o27, o27);
    o27 = smulm(o27, x7);
    int32_t hi = x7;
    for (int i = 0; i < 28; ++i) hi = smulm(hi, hi);
    return smulm(hi, o27);
}
PW_HD SExt sext_inv(const SExt& a) {
    const SExtInvPrep p = sext_inv_prepare(a);
    return sext_inv_finish(a, p, sinv(p.n));
}

// sum_k e_k t_k with e_k centred wave-uniform challenges and t_k in S: the seven coefficients of the product polynomial in int64 sums,
// 16 multiply-adds a term. Coefficient j takes min(j + 1, 7 - j) products per term, so it is folded after kAccPeriod{0,1,2,3} terms — as
// late as the int64 allows, each coefficient on its own schedule — where ExtProductAcc pays a 96-bit carry per coefficient and term.
struct SExtProductAcc {
    int64_t a[7];
    uint32_t n;  // terms so far (a compile-time constant in straight-line code)
    PW_HD SExtProductAcc() : a{0, 0, 0, 0, 0, 0, 0}, n(0) {}
    PW_HD void fold_due() {
        if (n == 0) return;
        if (n % bounds::kAccPeriod0 == 0) { a[0] = sfold(a[0]); a[6] = sfold(a[6]); }
        if (n % bounds::kAccPeriod1 == 0) { a[1] = sfold(a[1]); a[5] = sfold(a[5]); }
        if (n % bounds::kAccPeriod2 == 0) { a[2] = sfold(a[2]); a[4] = sfold(a[4]); }
        if (n % bounds::kAccPeriod3 == 0) a[3] = sfold(a[3]);
    }
    // e: centred coordinates of a wave-uniform element
    PW_HD void fma(const int32_t (&e)[4], const SExt& t) {
        fold_due();
        ++n;
        a[0] = swide_mad_uniform(a[0], t.c[0], e[0]);
        a[1] = swide_mad_uniform(swide_mad_uniform(a[1], t.c[1], e[0]), t.c[0], e[1]);
        a[2] = swide_mad_uniform(swide_mad_uniform(swide_mad_uniform(a[2], t.c[2], e[0]), t.c[1], e[1]), t.c[0], e[2]);
        a[3] = swide_mad_uniform(swide_mad_uniform(swide_mad_uniform(swide_mad_uniform(a[3], t.c[3], e[0]), t.c[2], e[1]), t.c[1], e[2]), t.c[0], e[3]);
        a[4] = swide_mad_uniform(swide_mad_uniform(swide_mad_uniform(a[4], t.c[3], e[1]), t.c[2], e[2]), t.c[1], e[3]);
        a[5] = swide_mad_uniform(swide_mad_uniform(a[5], t.c[3], e[2]), t.c[2], e[3]);
        a[6] = swide_mad_uniform(a[6], t.c[3], e[3]);
    }
    // canonical words of the sum: coefficients 4..6 come down once (they then carry R) and re-enter times 11 R
    PW_HD Ext result() {
#pragma unroll
        for (int k = 0; k < 7; ++k) a[k] = sfold(a[k]);
        Ext r;
#pragma unroll
        for (int k = 0; k < 3; ++k) r.c[k] = canonical_of_centred(smont(swide_mad_uniform(a[k], smont(a[4 + k]), kW11)));
        r.c[3] = canonical_of_centred(smont(a[3]));
        return r;
    }
};

// Inverse via the norm to the quadratic subfield K = F[Y]/(Y^2 - 11), Y = X^2:
// a = A0 + A1 X with A0 = (a0, a2), A1 = (a1, a3) in K; a^-1 = (A0 - A1 X) / (A0^2 - Y A1^2).
PW_HD Ext ext_inv(const Ext& a) {
    const uint32_t W = w11();
    // A0^2 = (a0^2 + 11 a2^2, 2 a0 a2), A1^2 = (a1^2 + 11 a3^2, 2 a1 a3)
    uint32_t s0 = add(sqr(a.c[0]), mul(W, sqr(a.c[2])));
    uint32_t s1 = double_(mul(a.c[0], a.c[2]));
    uint32_t t0 = add(sqr(a.c[1]), mul(W, sqr(a.c[3])));
    uint32_t t1 = double_(mul(a.c[1], a.c[3]));
    // D = A0^2 - Y*A1^2,  Y*(t0 + t1 Y) = 11 t1 + t0 Y
    uint32_t d0 = sub(s0, mul(W, t1));
    uint32_t d1 = sub(s1, t0);
    // D^-1 = (d0 - d1 Y) / (d0^2 - 11 d1^2)
    uint32_t n = sub(sqr(d0), mul(W, sqr(d1)));
    uint32_t ni = inv(n);
    uint32_t e0 = mul(d0, ni);
    uint32_t e1 = neg(mul(d1, ni));
    // R0 = A0 * E, R1 = -A1 * E  (K multiplication)
    uint32_t r00 = add(mul(a.c[0], e0), mul(W, mul(a.c[2], e1)));
    uint32_t r01 = add(mul(a.c[0], e1), mul(a.c[2], e0));
    uint32_t r10 = neg(add(mul(a.c[1], e0), mul(W, mul(a.c[3], e1))));
    uint32_t r11 = neg(add(mul(a.c[1], e1), mul(a.c[3], e0)));
    return {{r00, r10, r01, r11}};
}

PW_HD Ext ext_pow(Ext a, uint64_t e) {
    Ext r = ext_one();
    while (e) {
        if (e & 1) r = ext_mul(r, a);
        a = ext_sqr(a);
        e >>= 1;
    }
    return r;
}

}  // namespace bb
