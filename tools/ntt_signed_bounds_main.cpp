// The signed forward butterfly (bb::dit_signed, host path) at the edges of the ranges stated in csrc/ntt.hip (ntt::bounds) and on random
// triples, against plain 64-bit modular arithmetic. Header-only, no GPU:
//   c++ -std=c++17 -O1 -fsanitize=undefined tools/ntt_signed_bounds_main.cpp -o ntt_signed_bounds
//   ntt_signed_bounds <kInTop> <kTwiddleTop> <kSmontDomain> <kOutTop> [random triples = 1000000]
// For every (a, b, w, kappa) it checks that |a kappa + b w| and |a kappa - b w| lie inside the reduction's domain, that both outputs are
// below kOutTop in magnitude, and that X R = a kappa + b w, Y R = a kappa - b w (mod p) — with kappa = R mod p: X = a + b w, Y = a - b w
// as field elements in Montgomery form, which the random triples check through the canonical values as well. Prints the largest
// magnitudes it met; exit status 0 = every check held. tests/test_ntt_signed_bounds.py builds and runs it.
#include <cstdio>
#include <cstdlib>

#include "../powdr_amd/csrc/babybear.hpp"

namespace {

const int64_t kP = (int64_t)bb::P;
int64_t g_in_top, g_tw_top, g_domain, g_out_top;
int64_t g_max_wide = 0, g_max_out = 0;
long g_checked = 0;

int64_t mod_p(__int128 v) {
    int64_t r = (int64_t)(v % kP);
    return r < 0 ? r + kP : r;
}
int64_t mul_mod(int64_t a, int64_t b) { return (int64_t)((uint64_t)a * (uint64_t)b % (uint64_t)kP); }  // a, b in [0, p): a b < 2^62
int64_t pow_mod(int64_t a, uint64_t e) {
    int64_t r = 1;
    for (; e; e >>= 1, a = mul_mod(a, a))
        if (e & 1) r = mul_mod(r, a);
    return r;
}
int64_t mag(__int128 v) { return (int64_t)(v < 0 ? -v : v); }

bool fail(const char* what, int32_t a, int32_t b, int32_t w, int32_t k) {
    std::printf("FAILED %s: a=%d b=%d w=%d kappa=%d\n", what, a, b, w, k);
    return false;
}

bool check(int32_t a, int32_t b, int32_t w, int32_t k) {
    const __int128 tx = (__int128)a * k + (__int128)b * w, ty = (__int128)a * k - (__int128)b * w;
    if (mag(tx) >= g_domain || mag(ty) >= g_domain) return fail("|t| outside smont's domain", a, b, w, k);
    if (mag(tx) > g_max_wide) g_max_wide = mag(tx);
    if (mag(ty) > g_max_wide) g_max_wide = mag(ty);
    int32_t x = a, y = b;
    bb::dit_signed(x, y, w, -w, k);
    if (mag(x) >= g_out_top || mag(y) >= g_out_top) return fail("output outside kOutTop", a, b, w, k);
    if (mag(x) > g_max_out) g_max_out = mag(x);
    if (mag(y) > g_max_out) g_max_out = mag(y);
    const int64_t R = (int64_t)bb::R_MOD_P;
    if (mul_mod(mod_p(x), R) != mod_p(tx)) return fail("X R != a kappa + b w (mod p)", a, b, w, k);
    if (mul_mod(mod_p(y), R) != mod_p(ty)) return fail("Y R != a kappa - b w (mod p)", a, b, w, k);
    if (bb::canonical_of_centred(x) != (uint32_t)mod_p(x) || bb::canonical_of_centred(y) != (uint32_t)mod_p(y))
        return fail("canonical_of_centred", a, b, w, k);
    ++g_checked;
    return true;
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t next_u64() {  // splitmix64
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
int32_t uniform_sym(int64_t top_inclusive) { return (int32_t)((int64_t)(next_u64() % (uint64_t)(2 * top_inclusive + 1)) - top_inclusive); }

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) { std::printf("usage: %s kInTop kTwiddleTop kSmontDomain kOutTop [random triples]\n", argv[0]); return 2; }
    g_in_top = std::atoll(argv[1]);
    g_tw_top = std::atoll(argv[2]);
    g_domain = std::atoll(argv[3]);
    g_out_top = std::atoll(argv[4]);
    const long n_random = argc > 5 ? std::atol(argv[5]) : 1000000;
    if (g_tw_top != (kP - 1) / 2 || (int64_t)bb::R_MOD_P > g_tw_top) { std::printf("FAILED: twiddles are not centred\n"); return 1; }
    // the edge grid
    const int32_t e = (int32_t)(g_in_top - 1), h = (int32_t)g_tw_top;
    const int32_t ab[5] = {0, 1, -1, e, -e}, wk[5] = {h, -h, 1, -1, 0};
    for (int32_t a : ab)
        for (int32_t b : ab)
            for (int32_t w : wk)
                for (int32_t k : wk)
                    if (!check(a, b, w, k)) return 1;
    const int64_t edge_wide = g_max_wide, edge_out = g_max_out;
    // random triples under the kernel's kappa; the canonical values as well: X = a + b w, Y = a - b w for the field element w R^-1
    const int32_t kappa = (int32_t)bb::R_MOD_P;
    const int64_t rinv = pow_mod((int64_t)bb::R_MOD_P, (uint64_t)kP - 2);
    for (long i = 0; i < n_random; ++i) {
        const int32_t a = uniform_sym(g_in_top - 1), b = uniform_sym(g_in_top - 1), w = uniform_sym(g_tw_top);
        if (!check(a, b, w, kappa)) return 1;
        int32_t x = a, y = b;
        bb::dit_signed(x, y, w, -w);
        const int64_t bw = mul_mod(mod_p(b), mul_mod(mod_p(w), rinv));
        if (mod_p(x) != (mod_p(a) + bw) % kP || mod_p(y) != (mod_p(a) - bw + kP) % kP) {
            fail("X != a + b w or Y != a - b w", a, b, w, kappa);
            return 1;
        }
    }
    std::printf("ok checked=%ld edge_max_wide=%lld edge_max_out=%lld max_wide=%lld max_out=%lld\n", g_checked, (long long)edge_wide,
                (long long)edge_out, (long long)g_max_wide, (long long)g_max_out);
    return 0;
}
