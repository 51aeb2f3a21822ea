// Device-side helpers of the RUN-TIME SPECIALISED expression kernels (csrc/jit.hpp): this header, babybear.hpp and ext.hpp
// are embedded in libpowdr_gpu as text and handed to hiprtc together with the per-AIR source csrc/jit_codegen.cpp emits.
// The same functions are used by the ahead-of-time kernels of logup_kernels.hip, so the interpreter ("parity twin") and the
// specialised code share their arithmetic.
#pragma once
#include "ext.hpp"

namespace pwj {

using bb::Ext;

// trace cell (column base + byte offset of the row): `base` is wave-uniform (a scalar register pair), `off4` a 32-bit lane
// offset — the global_load form with a scalar base and a 32-bit vector offset, no 64-bit lane arithmetic per access
__device__ __forceinline__ uint32_t ld(const uint32_t* __restrict__ base, uint32_t off4) {
    return *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(base) + off4);
}
__device__ __forceinline__ void st(uint32_t* __restrict__ base, uint32_t off4, uint32_t v) {
    *reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(base) + off4) = v;
}

// d_i = al + bus_i + sum_j bl^(j+1) a_ij. Every coordinate is a sum of products accumulated RAW in a signed 64-bit register
// (one v_mad_i64_i32 per term): the challenge powers are wave-uniform, so their centred representatives (|b| <= p/2) come from
// the scalar unit for free, an argument a is a canonical word, a product is below p^2 / 2 and FOUR of them fit an int64 on top of
// what a fold leaves (bb::bounds::kDenTermsPerFold; <= 0.1422 p^2): after four products the accumulator is folded (bb::sfold, two
// instructions a coordinate), and the sum comes out through bb::smont_any as a class-S word whatever the term count was.
struct DenominatorSeeds {
    int64_t s[4];  // centred(al_k) * (R mod p): the value al_k in the accumulators' domain (k = 0: without the bus)
    uint32_t al0;
};
__device__ __forceinline__ DenominatorSeeds denominator_seeds(const Ext& al) {
    DenominatorSeeds sd;
#pragma unroll
    for (int k = 0; k < 4; ++k) sd.s[k] = (int64_t)bb::centred(al.c[k]) * (int64_t)bb::R_MOD_P;
    sd.al0 = al.c[0];
    return sd;
}
struct DenominatorAcc {
    int64_t T[4];
    uint32_t pending;
    __device__ __forceinline__ DenominatorAcc(const DenominatorSeeds& sd, uint32_t bus_monty)
        : T{(int64_t)bb::centred(bb::add(sd.al0, bus_monty)) * (int64_t)bb::R_MOD_P, sd.s[1], sd.s[2], sd.s[3]}, pending(0) {}
    __device__ __forceinline__ void fold() {
#pragma unroll
        for (int k = 0; k < 4; ++k) T[k] = bb::sfold(T[k]);
        pending = 0;
    }
    // argument j (canonical word a), b = bl^(j+1) (wave-uniform)
    __device__ __forceinline__ void add(uint32_t a, const Ext& b) {
        if (pending == (uint32_t)bb::bounds::kDenTermsPerFold) fold();
#pragma unroll
        for (int k = 0; k < 4; ++k) T[k] = bb::swide_mad_uniform(T[k], (int32_t)a, bb::centred(b.c[k]));
        ++pending;
    }
    __device__ __forceinline__ bb::SExt result_signed() const {
        return {{bb::smont_any(T[0]), bb::smont_any(T[1]), bb::smont_any(T[2]), bb::smont_any(T[3])}};
    }
    __device__ __forceinline__ Ext result() const { return bb::sext_canonical(result_signed()); }  // canonical words (the interpreters, the bus checks)
};
template <int NA>
__device__ __forceinline__ bb::SExt denominator(const DenominatorSeeds& sd, uint32_t bus_monty, const Ext* __restrict__ blpow, const uint32_t (&a)[NA]) {
    DenominatorAcc acc(sd, bus_monty);
#pragma unroll
    for (int j = 0; j < NA; ++j) acc.add(a[j], blpow[j + 1]);
    return acc.result_signed();
}
__device__ __forceinline__ bb::SExt denominator0(const DenominatorSeeds& sd, uint32_t bus_monty) {  // an interaction without arguments
    DenominatorAcc acc(sd, bus_monty);
    return acc.result_signed();
}

// d1 m0 + d0 m1 (the numerator of a two-member group; m0, m1 canonical words): the two products of a coordinate share one plain
// reduction; the result is a class-W word, the first operand of the products that follow
__device__ __forceinline__ bb::SExt scale2(const bb::SExt& a, uint32_t x, const bb::SExt& b, uint32_t y) {
    return bb::sext_scale2(a, bb::centred(x), b, bb::centred(y));
}

// Extension-field inversion split around its one base-field inversion (bb::sext_inv: norm to the quadratic subfield, then to
// the base field), so that several elements can share the ~70-product exponentiation (Montgomery's trick on the norms).
using ExtInvPrep = bb::SExtInvPrep;
__device__ __forceinline__ ExtInvPrep ext_inv_prepare(const bb::SExt& a) { return bb::sext_inv_prepare(a); }
__device__ __forceinline__ bb::SExt ext_inv_finish(const bb::SExt& a, const ExtInvPrep& p, int32_t n_inv) { return bb::sext_inv_finish(a, p, n_inv); }
// 1 / n[i] for K base-field elements (signed chain words, |n| <= bb::bounds::kChainMax: plain three-instruction products) with ONE
// inversion; a zero stays a zero's partner: the norm of an extension element is zero only for the zero element, whose inverse
// ext_inv_finish returns as zero whatever factor it is handed (bb::inv(0) = 0 in the one-by-one form), so a zero norm is replaced by
// one here. (A norm is below p in magnitude, so it is zero in the field only as the word 0.)
template <int K>
__device__ __forceinline__ void batch_inverse(const int32_t (&n)[K], int32_t (&out)[K]) {
    int32_t x[K], pre[K];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        x[i] = n[i] == 0 ? (int32_t)bb::R_MOD_P : n[i];
        pre[i] = i ? bb::smulm(pre[i - 1], x[i]) : x[i];
    }
    int32_t inv = bb::sinv(pre[K - 1]);
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
        out[i] = bb::smulm(inv, pre[i - 1]);
        inv = bb::smulm(inv, x[i]);
    }
    out[0] = inv;
}

// the centred coordinates of a wave-uniform element (scalar instructions)
struct Centred4 { int32_t c[4]; };
__device__ __forceinline__ Centred4 centred4(const Ext& e) { return {{bb::centred(e.c[0]), bb::centred(e.c[1]), bb::centred(e.c[2]), bb::centred(e.c[3])}}; }
// a permutation-matrix cell group (canonical words) as the centred first operand of q den
__device__ __forceinline__ bb::SExt ld_centred4(const uint32_t* __restrict__ base, size_t N, uint32_t off4) {
    return {{bb::centred(ld(base, off4)), bb::centred(ld(base + N, off4)), bb::centred(ld(base + 2 * N, off4)), bb::centred(ld(base + 3 * N, off4))}};
}
// sum of canonical words in a 64-bit register (one instruction a word) -> its canonical word, for up to 2^32 - 1 of them:
// monty_reduce takes t < p 2^32 and divides by R, the product by R^2 brings R back
__device__ __forceinline__ uint32_t reduce_word_sum(uint64_t t) { return bb::mul(bb::monty_reduce(t), bb::R2_MOD_P); }

}  // namespace pwj
