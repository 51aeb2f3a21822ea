// Stand-alone host check of the signed extension arithmetic (csrc/babybear.hpp: sfold / smont_any; csrc/ext.hpp: SExt and its
// operations; csrc/jit_device.hpp: the LogUp helpers on top of them) against the unsigned bb::ext_* functions, at the edges of every
// stated range (bb::bounds) and on random operands. Meant to be built with the host compiler and -fsanitize=address,undefined:
// the host forms of the primitives are plain signed sums, so an accumulator that leaves its int64 is reported by the sanitizer and
// shows as a wrong word as well. tests/test_ext_signed_bounds.py builds and runs it.
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ext_signed_selftest_main.cpp -o selftest && ./selftest
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline
#include "../powdr_amd/csrc/jit_device.hpp"

namespace {

using bb::Ext;
using bb::SExt;
namespace B = bb::bounds;

long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { fprintf(stderr, "FAILED %s:%d: %s | ", __FILE__, __LINE__, #cond); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return g_rng; }
int32_t rnd_in(int32_t bound) { return (int32_t)((int64_t)(rnd() % (2ull * (uint64_t)bound + 1)) - bound); }

uint32_t canon(int64_t x) { int64_t r = x % (int64_t)bb::P; return (uint32_t)(r < 0 ? r + bb::P : r); }
Ext canon(const SExt& a) { return {{canon(a.c[0]), canon(a.c[1]), canon(a.c[2]), canon(a.c[3])}}; }
bool in_class(const SExt& a, int32_t bound) { for (int k = 0; k < 4; ++k) if (a.c[k] > bound || a.c[k] < -bound) return false; return true; }
int64_t iabs(int64_t x) { return x < 0 ? -x : x; }

// ---- sfold / smont_any --------------------------------------------------------------------------------------------------------
void check_reduction(int64_t t) {
    const int64_t f = bb::sfold(t);
    CHECK(iabs(f) <= B::kSfoldMax, "sfold(%lld) = %lld", (long long)t, (long long)f);
    CHECK((uint32_t)(((__int128)t - f) % (int64_t)bb::P) == 0u, "sfold(%lld) is another residue", (long long)t);
    const int32_t r = bb::smont_any(t);
    CHECK(r <= B::kSmontAnyMax && r >= -B::kSmontAnyMax, "smont_any(%lld) = %d", (long long)t, r);
    CHECK((((__int128)r * 4294967296ll) - t) % (int64_t)bb::P == 0, "smont_any(%lld) = %d is not t / R", (long long)t, r);
}
void test_reductions() {
    const int64_t his[] = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    const uint64_t los[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (int64_t hi : his) for (uint64_t lo : los) check_reduction((int64_t)(((uint64_t)hi << 32) | lo));
    const int64_t more[] = {INT64_MIN, INT64_MAX, 0, 1, -1, B::kSmontDomain, -B::kSmontDomain, B::kSfoldMax, -B::kSfoldMax, B::kMulSumMax, -B::kMulSumMax};
    for (int64_t t : more) check_reduction(t);
    int32_t top = 0;
    int64_t ftop = 0;
    for (int i = 0; i < 1000000; ++i) {
        const int64_t t = (int64_t)rnd();
        check_reduction(t);
        const int32_t r = bb::smont_any(t);
        top = r > top ? r : -r > top ? -r : top;
        ftop = iabs(bb::sfold(t)) > ftop ? iabs(bb::sfold(t)) : ftop;
    }
    // plain smont at the ends of its domain
    for (int64_t t : {B::kSmontDomain, -B::kSmontDomain}) {
        const int32_t r = bb::smont(t);
        CHECK((((__int128)r * 4294967296ll) - t) % (int64_t)bb::P == 0, "smont at the end of its domain");
    }
    printf("sfold / smont_any: edges and 10^6 random int64; largest |smont_any| seen %.5f p (bound %.5f p), |sfold| %.5f p^2\n", top / (double)bb::P,
           B::kSmontAnyMax / (double)bb::P, ftop / (double)bb::P / bb::P);
}

// ---- the operations -----------------------------------------------------------------------------------------------------------
// a in class `ba`, b in class S, x and y centred
void check_ops(const SExt& a, const SExt& b, int32_t x, int32_t y, bool a_in_s) {
    const Ext A = canon(a), Bc = canon(b);
    const uint32_t X = canon(x), Y = canon(y);
    const bb::SExtB pb = bb::sext_prepare(b);
    for (int k = 0; k < 3; ++k) CHECK(pb.w[k] <= B::kPre11Max && pb.w[k] >= -B::kPre11Max && canon(pb.w[k]) == bb::mul(bb::w11(), Bc.c[k + 1]), "sext_prepare");
    const Ext AB = bb::ext_mul(A, Bc);
    SExt r = bb::sext_mul(a, pb);
    CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), AB), "sext_mul");
    CHECK(bb::ext_eq(canon(bb::sext_mul(a, b)), AB), "sext_mul (unprepared)");
    CHECK(bb::ext_eq(bb::sext_canonical(r), AB), "sext_canonical");
    r = bb::sext_mul_sub_base(a, pb, x);
    CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_sub(AB, bb::ext_from_base(X))), "sext_mul_sub_base");
    // the subtrahend of mul_sub may be a class-W word: a is one when !a_in_s
    r = bb::sext_mul_sub(b, pb, a);
    CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_sub(bb::ext_mul(Bc, Bc), A)), "sext_mul_sub");
    // num <- num d + den m: num = a (W or S), d = b, den in S
    const SExt den = a_in_s ? a : b;
    r = bb::sext_mul_add_scaled(a, pb, den, x);
    CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_add(AB, bb::ext_scale(canon(den), X))), "sext_mul_add_scaled");
    if (a_in_s) {
        r = bb::sext_sqr(a);
        CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_sqr(A)), "sext_sqr");
        r = bb::sext_scale(a, x);
        CHECK(in_class(r, B::kScaleMax) && bb::ext_eq(bb::sext_canonical(r), bb::ext_scale(A, X)), "sext_scale");
        r = bb::sext_scale2(a, x, b, y);
        CHECK(in_class(r, B::kWideMax) && bb::ext_eq(bb::sext_canonical(r), bb::ext_add(bb::ext_scale(A, X), bb::ext_scale(Bc, Y))), "sext_scale2");
        CHECK(bb::ext_eq(bb::sext_canonical(pwj::scale2(a, X, b, Y)), bb::ext_add(bb::ext_scale(A, X), bb::ext_scale(Bc, Y))), "pwj::scale2");
        const bb::SExtInvPrep ip = bb::sext_inv_prepare(a);
        CHECK(ip.n <= B::kNormMax && ip.n >= -B::kNormMax && ip.d0 <= B::kSmontAnyMax && ip.d0 >= -B::kSmontAnyMax && ip.d1 <= B::kSmontAnyMax && ip.d1 >= -B::kSmontAnyMax,
              "sext_inv_prepare's ranges");
        const int32_t ni = bb::sinv(ip.n);
        CHECK(ni <= B::kChainMax && ni >= -B::kChainMax && canon(ni) == bb::inv(canon(ip.n)), "sinv");
        r = bb::sext_inv_finish(a, ip, ni);
        CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_inv(A)), "sext_inv");
        CHECK(bb::ext_eq(canon(bb::sext_inv(a)), bb::ext_inv(A)), "sext_inv (whole)");
    }
    if (in_class(a, B::kHalf)) {  // q d0 d1 - (m0 d1 + m1 d0) in one reduction: q centred, the scaled words in S
        const SExt c = a_in_s ? a : b;
        r = bb::sext_mul_sub_scaled2(a, pb, c, x, b, y);
        CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), bb::ext_sub(AB, bb::ext_add(bb::ext_scale(canon(c), X), bb::ext_scale(Bc, Y)))), "sext_mul_sub_scaled2");
    }
    if (in_class(a, B::kHalf) && in_class(b, B::kHalf)) {
        CHECK(bb::ext_eq(bb::sext_canonical(bb::sext_add(a, b)), bb::ext_add(A, Bc)) && bb::ext_eq(bb::sext_canonical(bb::sext_sub(a, b)), bb::ext_sub(A, Bc)), "sext_add / sext_sub");
        CHECK(bb::ext_eq(bb::sext_canonical(bb::sext_centred(A)), A) && in_class(bb::sext_centred(A), B::kHalf), "sext_centred");
    }
}
void test_operations() {
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t ba = pass ? B::kWideMax : B::kSmontAnyMax;  // the first operand's class
        const int32_t ea[] = {0, 1, -1, B::kHalf, -B::kHalf, ba, -ba}, eb[] = {0, 1, -1, B::kHalf, -B::kHalf, B::kSmontAnyMax, -B::kSmontAnyMax};
        const int32_t ex[] = {0, 1, -1, B::kHalf, -B::kHalf};
        // every coordinate at an edge, all sign patterns of the bound among them
        for (int32_t va : ea) for (int32_t vb : eb) for (int32_t x : ex)
            check_ops({{va, va, va, va}}, {{vb, vb, vb, vb}}, x, -x, pass == 0);
        for (int sa = 0; sa < 16; ++sa) for (int sb = 0; sb < 16; ++sb) {
            SExt a, b;
            for (int k = 0; k < 4; ++k) { a.c[k] = (sa >> k & 1) ? -ba : ba; b.c[k] = (sb >> k & 1) ? -B::kSmontAnyMax : B::kSmontAnyMax; }
            for (int32_t x : ex) check_ops(a, b, x, x, pass == 0);
        }
        // an edge in every coordinate position of either operand, the others random
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) for (int32_t va : ea) for (int32_t vb : eb) {
            SExt a, b;
            for (int k = 0; k < 4; ++k) { a.c[k] = rnd_in(ba); b.c[k] = rnd_in(B::kSmontAnyMax); }
            a.c[i] = va;
            b.c[j] = vb;
            check_ops(a, b, ex[(i + j) % 5], ex[(i * 4 + j) % 5], pass == 0);
        }
        for (int n = 0; n < 1000000; ++n) {
            SExt a, b;
            for (int k = 0; k < 4; ++k) { a.c[k] = rnd_in(ba); b.c[k] = rnd_in(B::kSmontAnyMax); }
            check_ops(a, b, rnd_in(B::kHalf), rnd_in(B::kHalf), pass == 0);
        }
    }
    // what an EMPTY group would compute (logup_group_starts never makes one, so no kernel test reaches these lines of the generators and
    // of the interpreter twins): den = 1, num = 0 — the quotient's term q 1 - 0 = q, the permutation's inverse of one, its column zero
    CHECK(bb::ext_eq(bb::sext_canonical(bb::sext_one()), bb::ext_one()) && bb::ext_eq(bb::sext_canonical(bb::sext_zero()), bb::ext_zero()), "one and zero");
    for (int32_t v : {0, 1, -1, B::kHalf, -B::kHalf}) {
        const SExt q = {{v, -v, v / 2, v}};
        CHECK(bb::ext_eq(canon(bb::sext_mul_sub(q, bb::sext_prepare(bb::sext_one()), bb::sext_zero())), canon(q)), "an empty group's quotient term is q");
    }
    {
        const bb::SExtInvPrep ip = bb::sext_inv_prepare(bb::sext_one());
        const int32_t n[1] = {ip.n};
        int32_t ni[1];
        pwj::batch_inverse<1>(n, ni);
        CHECK(bb::ext_eq(canon(bb::sext_inv_finish(bb::sext_one(), ip, ni[0])), bb::ext_one()), "an empty group's denominator one has the inverse one");
    }
    // zero has the inverse zero, also inside a batch
    CHECK(bb::ext_eq(canon(bb::sext_inv(bb::sext_zero())), bb::ext_zero()), "the inverse of zero");
    for (int zero_at = -1; zero_at < 4; ++zero_at) {
        int32_t n[4], out[4];
        for (int k = 0; k < 4; ++k) n[k] = k == zero_at ? 0 : (k & 1 ? -B::kNormMax : B::kNormMax) + k;
        pwj::batch_inverse<4>(n, out);
        for (int k = 0; k < 4; ++k) {
            CHECK(out[k] <= B::kChainMax && out[k] >= -B::kChainMax, "batch_inverse's range");
            CHECK(k == zero_at || canon(out[k]) == bb::inv(canon(n[k])), "batch_inverse");
        }
    }
    printf("signed product, square, scale, scale2, inverse, fused forms: edges in every position and 2 x 10^6 random operands\n");
}

// ---- the accumulators ---------------------------------------------------------------------------------------------------------
void test_accumulators() {
    // denominators: seed and terms at their bounds, 0 .. 3 folds and one term beyond each. all_top: EVERY argument is p - 1 and every
    // challenge coordinate has one sign, so each run of kDenTermsPerFold terms piles kDenTermsPerFold * kDenTerm of one sign on top of
    // what the fold left — the int64 headroom the term count claims, under the sanitizer; otherwise every third argument is random
    int64_t den_top = 0;
    for (int all_top = 0; all_top < 2; ++all_top) for (int sign = 0; sign < 4; ++sign) for (int n_args = 0; n_args <= 3 * B::kDenTermsPerFold + 1; ++n_args) {
        const uint32_t al_w = sign & 1 ? (uint32_t)B::kHalf : (uint32_t)B::kHalf + 1u, b_w = sign & 2 ? (uint32_t)B::kHalf : (uint32_t)B::kHalf + 1u;  // centred: +-(p-1)/2
        const Ext al = {{al_w, al_w, al_w, al_w}}, bl = {{b_w, b_w, b_w, b_w}};
        const pwj::DenominatorSeeds sd = pwj::denominator_seeds(al);
        pwj::DenominatorAcc acc(sd, 0u);
        Ext want = al;
        for (int j = 0; j < n_args; ++j) {
            const uint32_t a = !all_top && j % 3 == 2 ? (uint32_t)rnd_in(B::kHalf) + (uint32_t)B::kHalf : bb::P - 1;
            acc.add(a, bl);
            for (int k = 0; k < 4; ++k) {
                CHECK(iabs(acc.T[k]) <= B::kSfoldMax + (int64_t)acc.pending * B::kDenTerm, "DenominatorAcc's sums, %d arguments", j + 1);
                den_top = iabs(acc.T[k]) > den_top ? iabs(acc.T[k]) : den_top;
            }
            want = bb::ext_add(want, bb::ext_scale(bl, a));
        }
        const SExt r = acc.result_signed();
        CHECK(in_class(r, B::kSmontAnyMax) && bb::ext_eq(canon(r), want) && bb::ext_eq(acc.result(), want), "DenominatorAcc with %d arguments", n_args);
    }
    // the fullest sum seen must BE a full run at the bound on top of a folded value: at least the terms alone
    CHECK(den_top >= (int64_t)B::kDenTermsPerFold * B::kDenTerm && den_top <= B::kSfoldMax + (int64_t)B::kDenTermsPerFold * B::kDenTerm, "the fullest denominator sum");
    printf("denominator sums: fullest |T| = %.4f p^2 = %.4f of the int64 range\n", (double)den_top / bb::P / bb::P, (double)den_top / 9223372036854775807.0);
    // centred sums: the callers' four terms between folds, and the eight the bounds allow
    for (int per_fold : {4, B::kCentredTermsPerFold}) for (int n = 0; n <= 3 * per_fold + 1; ++n) for (int sign = 0; sign < 2; ++sign) {
        bb::ExtCentredAcc acc;
        const int32_t e[4] = {B::kHalf, -B::kHalf, B::kHalf, -B::kHalf};
        Ext want = bb::ext_zero();
        for (int k = 0; k < n; ++k) {
            if (k && k % per_fold == 0) acc.fold();
            const int32_t x = sign ? -B::kHalf : B::kHalf;
            acc.fma(e, x);
            want = bb::ext_add(want, bb::ext_scale(canon(SExt{{e[0], e[1], e[2], e[3]}}), canon(x)));
        }
        CHECK(bb::ext_eq(acc.result(), want), "ExtCentredAcc, %d terms, a fold every %d", n, per_fold);
    }
    // product sums: challenge coordinates and term words at their bounds, past two folds of the slowest coefficient
    for (int sign = 0; sign < 4; ++sign) for (int n = 0; n <= 2 * B::kAccPeriod0 + 1; ++n) {
        bb::SExtProductAcc acc;
        bb::ExtProductAcc ref;
        const int32_t ev = sign & 1 ? -B::kHalf : B::kHalf, tv = sign & 2 ? -B::kSmontAnyMax : B::kSmontAnyMax;
        for (int k = 0; k < n; ++k) {
            const int32_t e[4] = {ev, ev, ev, ev};
            SExt t = {{tv, tv, tv, tv}};
            if (k % 5 == 4) for (int c = 0; c < 4; ++c) t.c[c] = rnd_in(B::kSmontAnyMax);
            acc.fma(e, t);
            ref.fma(canon(SExt{{e[0], e[1], e[2], e[3]}}), canon(t));
        }
        CHECK(bb::ext_eq(acc.result(), ref.result()), "SExtProductAcc, %d terms", n);
    }
    for (int n = 0; n < 200000; ++n) {
        bb::SExtProductAcc acc;
        bb::ExtProductAcc ref;
        const int terms = (int)(rnd() % 24);
        for (int k = 0; k < terms; ++k) {
            int32_t e[4];
            SExt t;
            for (int c = 0; c < 4; ++c) { e[c] = rnd_in(B::kHalf); t.c[c] = rnd_in(B::kSmontAnyMax); }
            acc.fma(e, t);
            ref.fma(canon(SExt{{e[0], e[1], e[2], e[3]}}), canon(t));
        }
        CHECK(bb::ext_eq(acc.result(), ref.result()), "SExtProductAcc, random, %d terms", terms);
    }
    for (uint64_t words : std::vector<uint64_t>{0u, 1u, (uint64_t)bb::P - 1, (uint64_t)bb::P, ((uint64_t)bb::P - 1) * 0xffffffffull})
        CHECK(pwj::reduce_word_sum(words) == (uint32_t)(words % bb::P), "reduce_word_sum");
    printf("accumulators: denominators, centred sums and product sums filled to their term counts at the bounds and beyond a fold\n");
}

}  // namespace

int main() {
    test_reductions();
    test_operations();
    test_accumulators();
    printf("ext_signed_selftest: %ld checks passed\n", g_checks);
    return 0;
}
