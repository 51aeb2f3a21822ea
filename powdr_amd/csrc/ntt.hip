// Radix-2 NTT / low-degree extension over BabyBear for gfx950: LDS-staged stage groups with
// register-resident radix-16 rounds.
//
// Column-major matrices of 2^n-row columns; every column is an independent transform
// (blockIdx.y = column). A transform of n stages is cut into "stage groups": one launch runs k
// consecutive butterfly stages on a tile of 2^(k+c) elements, so the data crosses HBM once per
// group, not once per stage. A tile gathers the 2^k elements whose indices differ in the
// group's k active bits, times 2^c neighbouring elements (c low index bits) so that every global
// access of a strided group is a contiguous segment of 64 bytes (128 for tall transforms: plan_groups).
//
// Inside a group a "round" runs up to 4 stages without touching LDS: a thread holds a "slot", the
// 2^logr <= 16 elements of a radix-16 butterfly network, in VGPRs, and takes the 16 (2^12-element
// tile) or 32 (2^13) elements it owns per round one slot after the other; rounds exchange data
// through a padded LDS tile (one extra word per 32: conflict-free for every round's access pattern). The
// first round of a group loads straight from HBM into registers and the last round stores
// straight from registers to HBM. Twiddles: the factor of a butterfly splits into a per-thread
// base (one table lookup per slot, squared from stage to stage) times a constant 16th/8th/4th
// root of unity, so no per-butterfly table traffic exists; groups whose factors do not depend on
// the tile read all of a slot's twiddles from a small per-group table instead (group_twiddles).
//
//   inverse  = DIF (Gentleman-Sande), natural-order input -> bit-reversed output
//   forward  = DIT (Cooley-Tukey),    bit-reversed input  -> natural-order output
// so iNTT followed by the coset NTT needs no bit-reversal pass. Zero-padding the coefficient
// vector from H to 2H in bit-reversed order is a duplication (padded[2q] = c[q], padded[2q+1] = 0,
// and the first DIT stage maps (a, 0) to (a, a)); the first DIT group of the LDE reads the
// H-sized coefficient array directly, applies the coset scaling s^k/H and duplicates in
// registers (EXPAND), so the 2H-sized vector is written exactly once per group.
//
// LDE definition (natural order, as oracle/stark_oracle.cpp `lde_column`):
//   L[j] = T(s * g_{n+1}^j),  j < 2H,  s = 31.
#include "babybear.hpp"
#include "common.hpp"
#include "prover_internal.hpp"

#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>
#include <vector>

namespace pw {

namespace {

constexpr int kBlock = 256;
__constant__ uint32_t c_roots16[2][8];  // [0]: w16^r forward, [1]: inverse (Montgomery), r < 8

__global__ void fill_powers_kernel(uint32_t* out, uint32_t base, uint32_t scale, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = bb::mul(bb::pow_u32(base, (uint32_t)i), scale);
}
__global__ void bitrev_copy_kernel(const uint32_t* in, uint32_t* out, int n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ((size_t)1 << n)) return;
    uint32_t k = n ? (__brev((uint32_t)i) >> (32 - n)) : 0u;
    out[i] = in[k];
}

struct GroupParams {
    int n;        // log2 of the transform size
    int s0;       // first stage of the group
    int k;        // stages in the group
    int c;        // passive low bits carried in the tile
    int lowbits;  // index bits below the active bits (DIF: n-s0-k, DIT: s0)
    int B;        // k + c: in-tile index bits
    int n_rounds;
    int rb[4];    // window start (tile bit) per round, in execution order
    int logr[4];  // window width per round
    unsigned long long n_tiles;  // tiles per column = 2^(n-B)
    int canonical_out;  // forward transform: the last group reduces its [0, 2p) values to [0, p) when it stores
    unsigned twt_off[4];  // per round: offset of its twiddle table (tile-invariant groups: group_twiddles, FusedTwiddles)
    // sub-coset evaluation (subcoset_lde): FOLD loads — element g of the transform's input is the sum of 2^fold coefficients times the
    // wave-uniform constants foldk[] — and a COSET transform: the twiddles of stage s carry the constant c^(2^(n-1-s)). Tile-invariant
    // groups read them from a table derived for the sub-coset; the others multiply a round's top twiddle base by cst[round] (the lower
    // stages' constants follow from the squaring chain).
    int fold;
    int coset;
    uint32_t foldk[16];
    uint32_t cst[4];
    // SELECT (the query phase of a streamed proof, subcoset_query_rows): the group's outputs are not stored — of every tile only the
    // n_sel positions sel_pos[q] are used: the term position * sel_xpow[q * n_tiles + tile] of output q goes to
    // sel_part[(column * n_tiles + tile) * n_sel + q] (one plain store per term; select_reduce_kernel sums a column's tiles) — or, with
    // sel_part == nullptr (POWDR_QUERY_SELECT=2, round 5's form), is added to sel_acc[column * n_sel + q] by a 64-bit atomic.
    int n_sel;
    const uint32_t* sel_pos;
    const uint32_t* sel_xpow;
    unsigned long long* sel_acc;
    uint32_t* sel_part;
};

__device__ __forceinline__ uint32_t lds_phys(uint32_t l) { return l + (l >> 5); }

struct IndexMap {
    int B, c, lowbits, k;
    uint32_t cmask;
    size_t tile0;
    size_t n_tiles;
    // global index of local element l; valid = tile exists
    __device__ __forceinline__ size_t global(uint32_t l, bool& valid) const {
        const uint32_t i = l & ((1u << B) - 1u);
        const size_t tile = tile0 + (l >> B);
        valid = tile < n_tiles;
        const int lo_hi_bits = lowbits - c;
        const size_t lo_hi = tile & (((size_t)1 << lo_hi_bits) - 1);
        const size_t hi = tile >> lo_hi_bits;
        return (hi << (lowbits + k)) | ((size_t)(i >> c) << lowbits) | (lo_hi << c) | (size_t)(i & cmask);
    }
    // global index bits below tile bit `rb` for the slot whose local index (with the window zeroed) is l
    __device__ __forceinline__ size_t glow(uint32_t l, int rb) const {
        const uint32_t i = l & ((1u << rb) - 1u);
        const size_t tile = tile0 + (l >> B);
        if (tile >= n_tiles) return 0;  // padding slot of a short transform: any in-range twiddle
        const int lo_hi_bits = lowbits - c;
        const size_t lo_hi = tile & (((size_t)1 << lo_hi_bits) - 1);
        return ((size_t)(i >> c) << lowbits) | (lo_hi << c) | (size_t)(i & cmask);
    }
};

// One slot of one round: LOGR stages on the window [rb, rb+LOGR) of the tile index, on the
// R = 2^LOGR elements v[rho] (fully reduced arithmetic: see the note at bb::mul_lazy).
// The twiddle base of slot m of a round: w^(g << shift) for the slot's low global index bits g and the round's
// smallest shift (the one of window bit logr-1). A table lookup with global-memory latency on the critical path
// of the slot's butterflies, so callers fetch it one slot (or one round) ahead.
template <bool DIF>
__device__ __forceinline__ uint32_t load_twiddle_base(const IndexMap& im, const GroupParams& gp, int round, int m, int tid,
                                                      const uint32_t* __restrict__ tw) {
    const int rb = gp.rb[round], logr = gp.logr[round];
    const uint32_t sigma = (uint32_t)tid + (uint32_t)kBlock * m;
    const uint32_t l0 = ((sigma >> rb) << (rb + logr)) | (sigma & ((1u << rb) - 1u));
    const size_t g = im.glow(l0, rb);
    const int sh_top = DIF ? gp.s0 + gp.k - 1 - (rb + (logr - 1) - gp.c)       // stage number s_q
                           : gp.n - 1 - (gp.s0 + rb + (logr - 1) - gp.c);       // n - 1 - s_q
    return tw[g << sh_top];
}

// `tt` (TWT): the slot's 2^LOGR - 1 twiddles, stage q at [2^q - 1, 2^(q+1) - 1), loaded from a table instead of being derived
// from `base_top` by LOGR - 1 squarings and 2^LOGR - 1 - LOGR products (70 of a radix-16 slot's 390 instructions).
template <bool DIF, int LOGR, bool TWT = false>
__device__ __forceinline__ void slot_butterflies(uint32_t* v, uint32_t base_top, const uint32_t* tt = nullptr) {
    constexpr int R = 1 << LOGR;
    const uint32_t* roots = c_roots16[DIF ? 1 : 0];
    // base[q] = w^(g << shift_q); the smallest shift belongs to q = LOGR-1 and base[q-1] = base[q]^2
    uint32_t base[LOGR];
    if (!TWT) {
        base[LOGR - 1] = base_top;
#pragma unroll
        for (int q = LOGR - 2; q >= 0; --q) base[q] = bb::sqr(base[q + 1]);
    }
#pragma unroll
    for (int qi = 0; qi < LOGR; ++qi) {
        const int q = DIF ? (LOGR - 1 - qi) : qi;
        // twiddles of this stage: base[q] * w_{2^(q+1)}^r, r < 2^q;  w_{2^(q+1)}^r = w16^(r << (3 - q))
        uint32_t t[1 << (LOGR - 1)], nt[1 << (LOGR - 1)];
#pragma unroll
        for (int r = 0; r < (1 << q); ++r) {
            if (TWT) t[r] = tt[(1 << q) - 1 + r];
            else t[r] = r == 0 ? base[q] : bb::mul(base[q], roots[r << (3 - q)]);
            if (DIF) nt[r] = bb::P - t[r];  // a representative of -t in (0, p]: fine as a factor
        }
#pragma unroll
        for (int u = 0; u < R / 2; ++u) {
            const int lowp = u & ((1 << q) - 1);
            const int i0 = ((u >> q) << (q + 1)) | lowp;
            const int i1 = i0 | (1 << q);
            const uint32_t a = v[i0], b = v[i1];
            if (DIF) {
                v[i0] = bb::add(a, b);
                v[i1] = bb::mul2(a, t[lowp], b, nt[lowp]);  // (a - b) t as a t + b (p - t): one reduction, no subtraction
            } else {
                // forward transform: all values are representatives in [0, 2p) between the first load and the last store
                const uint32_t bt = bb::mul_lazy(b, t[lowp]);
                v[i0] = bb::add_2p(a, bt);
                v[i1] = bb::sub_2p(a, bt);
            }
        }
    }
}

// FOLD load (sub-coset evaluation, subcoset_lde below): input element g of a size-2^n' transform is
//   sum_{t < 2^f} src[(g << f) + t] * K[t]
// — the polynomial reduced modulo x^(2^n') - c^(2^n') on the sub-coset, in bit-reversed order: the 2^f coefficients that fold onto one
// position are contiguous, and their factors (c^(2^n') to the power bitrev(t), over H) are the same for every position. Canonical.
__device__ __forceinline__ uint32_t fold_load(const uint32_t* __restrict__ src, const uint32_t* K, size_t g, int f) {
    const size_t q = g << f;
    if (f == 0) return bb::mul(src[q], K[0]);
    if (f == 1) {
        const uint2 a = *reinterpret_cast<const uint2*>(src + q);
        return bb::mul2(a.x, K[0], a.y, K[1]);
    }
    const uint4* pa = reinterpret_cast<const uint4*>(src + q);
    uint32_t acc = 0u;
    for (int t = 0; t < (1 << (f - 2)); ++t) {
        const uint4 a = pa[t];
        acc = bb::add(acc, bb::add(bb::mul2(a.x, K[4 * t], a.y, K[4 * t + 1]), bb::mul2(a.z, K[4 * t + 2], a.w, K[4 * t + 3])));
    }
    return acc;
}

// One round of a group, slot by slot (a slot = the R elements a thread combines). A round is an
// in-place network: every slot reads and writes the same R tile positions, so slots need no
// barrier among themselves; barriers separate rounds only. The first round of a group loads from
// HBM, the last one stores to HBM.
// EXPAND: `src` is the H-sized bit-reversed coefficient array (n = log2(2H)); element g of the
// 2H-sized vector is src[g >> 1] * scale_br[g >> 1].
// `tw_base` enters as the twiddle base of this round's slot 0 and leaves as the one of the next round's slot 0.
// MODE: 0 = plain loads, 1 = EXPAND, 2 = FOLD (fold_load above). EPT: the elements a thread owns (tile size / kBlock).
template <bool DIF, int LOGR, int EPT, int MODE, bool TWT = false>
__device__ __forceinline__ void run_round(uint32_t* tile, const IndexMap& im, const GroupParams& gp, int round,
                                          const uint32_t* __restrict__ src, uint32_t* __restrict__ dst,
                                          const uint32_t* __restrict__ tw, const uint32_t* __restrict__ scale_br, int tid,
                                          uint32_t& tw_base, bool io_first = true, bool io_last = true) {
    constexpr bool EXPAND = MODE == 1, FOLD = MODE == 2;
    const int rb = gp.rb[round];
    // io_first / io_last = false: the group's first round reads / its last round writes the LDS tile instead of HBM
    // (the fused LDE kernel chains two groups through LDS)
    const bool last_round = round == gp.n_rounds - 1;
    const bool first = round == 0 && io_first, last = last_round && io_last;
    constexpr int R = 1 << LOGR;
    constexpr int SLOTS = EPT / R;
    const bool vec_plain = rb == 0 && gp.c == 0 && LOGR >= 2;   // the slot's elements are contiguous in HBM
    const bool vec_expand = EXPAND && rb == 1 && gp.c == 1 && LOGR >= 2;
    const int gshift = rb - gp.c + gp.lowbits;
    // padded LDS position of element rho of a slot, relative to the slot's base: the window bits and the
    // slot's bits are disjoint, so lds_phys(l0 | rho << rb) = lds_phys(l0) + lds_off(rho); wave-uniform
    auto lds_off = [rb](int rho) -> uint32_t {
        return ((uint32_t)rho << rb) + (rb >= 5 ? ((uint32_t)rho << (rb - 5)) : ((uint32_t)rho >> (5 - rb)));
    };
#pragma unroll 1
    for (int m = 0; m < SLOTS; ++m) {
        const uint32_t sigma = (uint32_t)tid + (uint32_t)kBlock * m;
        const uint32_t l0 = ((sigma >> rb) << (rb + LOGR)) | (sigma & ((1u << rb) - 1u));
        const uint32_t p0 = lds_phys(l0);
        // fetch the next slot's (or the next round's first) twiddle base while this slot computes
        const uint32_t cur_base = (!TWT && gp.coset) ? bb::mul(tw_base, gp.cst[round]) : tw_base;
        uint32_t tt[R];  // TWT: the slot's twiddles from the group's table (`tw`), [stage-major index][g], g = the index bits below the window
        if (TWT) {
            const uint32_t* tab = tw + gp.twt_off[round] + (l0 & ((1u << rb) - 1u));
#pragma unroll
            for (int j = 0; j < R - 1; ++j) tt[j] = tab[(uint32_t)j << rb];
        } else {
            if (m + 1 < SLOTS) tw_base = load_twiddle_base<DIF>(im, gp, round, m + 1, tid, tw);
            else if (!last_round) tw_base = load_twiddle_base<DIF>(im, gp, round + 1, 0, tid, tw);
        }
        uint32_t x[R];
        // ---- load ----
        if (first) {
            if (FOLD) {
                bool valid;
                const size_t g0 = im.global(l0, valid);
                if (valid) {
#pragma unroll
                    for (int rho = 0; rho < R; ++rho) x[rho] = fold_load(src, gp.foldk, g0 + ((size_t)rho << gshift), gp.fold);
                } else {
#pragma unroll
                    for (int rho = 0; rho < R; ++rho) x[rho] = 0u;
                }
            } else if (EXPAND ? vec_expand : vec_plain) {
                bool valid;
                const size_t g0 = im.global(l0, valid);
                const uint4* pc = reinterpret_cast<const uint4*>(src + (EXPAND ? (g0 >> 1) : g0));
                const uint4* ps = reinterpret_cast<const uint4*>(scale_br + (g0 >> 1));
#pragma unroll
                for (int v4 = 0; v4 < R / 4; ++v4) {
                    uint4 d = make_uint4(0, 0, 0, 0);
                    if (valid) d = pc[v4];
                    if (EXPAND) {
                        uint4 sc = make_uint4(0, 0, 0, 0);
                        if (valid) sc = ps[v4];
                        d.x = bb::mul(d.x, sc.x); d.y = bb::mul(d.y, sc.y); d.z = bb::mul(d.z, sc.z); d.w = bb::mul(d.w, sc.w);
                    }
                    x[4 * v4 + 0] = d.x; x[4 * v4 + 1] = d.y; x[4 * v4 + 2] = d.z; x[4 * v4 + 3] = d.w;
                }
            } else {
                // window bit (rb + q) of the tile index is bit gshift + q of the global index
                bool valid;
                const size_t g0 = im.global(l0, valid);
                if (EXPAND) {
                    const size_t q0 = g0 >> 1;
                    const int qshift = gshift - 1;  // the EXPAND group has lowbits = c = 1, so gshift = rb >= 1
                    // one test per slot, not one predicated load per element: the R loads issue back to back
                    if (valid) {
                        uint32_t cf[R], sc[R];
#pragma unroll
                        for (int rho = 0; rho < R; ++rho) { const size_t q = q0 + ((size_t)rho << qshift); cf[rho] = src[q]; sc[rho] = scale_br[q]; }
#pragma unroll
                        for (int rho = 0; rho < R; ++rho) x[rho] = bb::mul(cf[rho], sc[rho]);
                    } else {
#pragma unroll
                        for (int rho = 0; rho < R; ++rho) x[rho] = 0u;
                    }
                } else {
                    const uint32_t* ps = src + g0;
                    if (valid) {
#pragma unroll
                        for (int rho = 0; rho < R; ++rho) x[rho] = ps[(size_t)rho << gshift];
                    } else {
#pragma unroll
                        for (int rho = 0; rho < R; ++rho) x[rho] = 0u;
                    }
                }
            }
        } else {
#pragma unroll
            for (int rho = 0; rho < R; ++rho) x[rho] = tile[p0 + lds_off(rho)];
        }
        // ---- butterflies ----
        slot_butterflies<DIF, LOGR, TWT>(x, cur_base, tt);
        // ---- store ----
        if (!DIF && last && gp.canonical_out) {
#pragma unroll
            for (int rho = 0; rho < R; ++rho) x[rho] = bb::reduce_2p(x[rho]);
        }
        if (last) {
            if (vec_plain) {
                bool valid;
                const size_t g0 = im.global(l0, valid);
                if (valid) {
                    uint4* pd = reinterpret_cast<uint4*>(dst + g0);
#pragma unroll
                    for (int v4 = 0; v4 < R / 4; ++v4) pd[v4] = make_uint4(x[4 * v4], x[4 * v4 + 1], x[4 * v4 + 2], x[4 * v4 + 3]);
                }
            } else {
                bool valid;
                const size_t g0 = im.global(l0, valid);
                if (valid) {
                    uint32_t* pd = dst + g0;
#pragma unroll
                    for (int rho = 0; rho < R; ++rho) pd[(size_t)rho << gshift] = x[rho];
                }
            }
        } else {
#pragma unroll
            for (int rho = 0; rho < R; ++rho) tile[p0 + lds_off(rho)] = x[rho];
        }
    }
}

// TWT: `tw` is the group's twiddle TABLE (tile-invariant groups, see group_twiddles) instead of the transform's root table
template <bool DIF, int LOGT, int MODE, bool TWT = false>
__global__ __launch_bounds__(kBlock) void ntt_group_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                           size_t in_stride, size_t out_stride, GroupParams gp,
                                                           const uint32_t* __restrict__ tw,
                                                           const uint32_t* __restrict__ scale_br) {
    constexpr int EPT = (1 << LOGT) / kBlock;
    __shared__ uint32_t tile[(1 << LOGT) + ((1 << LOGT) >> 5)];
    const int tid = threadIdx.x;
    IndexMap im;
    im.B = gp.B; im.c = gp.c; im.lowbits = gp.lowbits; im.k = gp.k;
    im.cmask = (1u << gp.c) - 1u;
    im.tile0 = (size_t)blockIdx.x << (LOGT - gp.B);
    im.n_tiles = (size_t)gp.n_tiles;
    const uint32_t* src = in + (size_t)blockIdx.y * in_stride;
    uint32_t* dst = out + (size_t)blockIdx.y * out_stride;
    uint32_t tw_base = TWT ? 0u : load_twiddle_base<DIF>(im, gp, 0, 0, tid, tw);
    // FOLD (sub-coset evaluation): the folded inputs of the workgroup's tile(s) are staged through LDS first — lane = output, so a wave
    // reads 2^fold * 256 CONTIGUOUS bytes per instruction. (Loaded slot by slot like the other modes, a lane would read the 16 neighbouring
    // outputs of its slot: 64 lanes x 16 instructions walking 64 cache lines side by side, which L1 does not hold for a CU's worth of waves.)
    constexpr bool kStageFold = MODE == 2;
    const bool select = MODE == 2 && gp.n_sel > 0;
    if (kStageFold) {
        if (gp.B == LOGT && gp.c == 0 && gp.lowbits == 0 && gp.fold <= 1) {
            // The whole-tile case of a tall transform (one tile per workgroup, element l of the tile = element tile * 2^LOGT + l of the
            // transform's input): every lane issues ALL its loads — 16 bytes each — before the first product, instead of four 4-byte
            // loads at a time (round 5: the group ran at 56 % of the issue rate with 30 % of the HBM rate, waiting for its own loads).
            const size_t g0 = (size_t)blockIdx.x << LOGT;
            constexpr int kVec = (1 << LOGT) / (4 * kBlock);  // uint4 loads per lane and coefficient word of an output
            if (gp.fold == 0) {
                const uint4* pv = reinterpret_cast<const uint4*>(src + g0);
                uint4 d[kVec];
#pragma unroll
                for (int m = 0; m < kVec; ++m) d[m] = pv[(uint32_t)tid + kBlock * m];
                const uint32_t k0 = gp.foldk[0];
#pragma unroll
                for (int m = 0; m < kVec; ++m) {
                    const uint32_t l = 4u * ((uint32_t)tid + kBlock * m);
                    tile[lds_phys(l)] = bb::mul(d[m].x, k0); tile[lds_phys(l + 1)] = bb::mul(d[m].y, k0);
                    tile[lds_phys(l + 2)] = bb::mul(d[m].z, k0); tile[lds_phys(l + 3)] = bb::mul(d[m].w, k0);
                }
            } else {  // two coefficient words per output: a uint4 holds two outputs
                const uint4* pv = reinterpret_cast<const uint4*>(src + 2 * g0);
                uint4 d[2 * kVec];
#pragma unroll
                for (int m = 0; m < 2 * kVec; ++m) d[m] = pv[(uint32_t)tid + kBlock * m];
                const uint32_t k0 = gp.foldk[0], k1 = gp.foldk[1];
#pragma unroll
                for (int m = 0; m < 2 * kVec; ++m) {
                    const uint32_t l = 2u * ((uint32_t)tid + kBlock * m);
                    tile[lds_phys(l)] = bb::mul2(d[m].x, k0, d[m].y, k1);
                    tile[lds_phys(l + 1)] = bb::mul2(d[m].z, k0, d[m].w, k1);
                }
            }
        } else {
#pragma unroll 4
            for (uint32_t l = (uint32_t)tid; l < (1u << LOGT); l += kBlock) {
                bool valid;
                const size_t g = im.global(l, valid);
                tile[lds_phys(l)] = valid ? fold_load(src, gp.foldk, g, gp.fold) : 0u;
            }
        }
        __syncthreads();
    }
    for (int r = 0; r < gp.n_rounds; ++r) {
        switch (gp.logr[r]) {
            case 1: run_round<DIF, 1, EPT, MODE, TWT>(tile, im, gp, r, src, dst, tw, scale_br, tid, tw_base, !kStageFold, !select); break;
            case 2: run_round<DIF, 2, EPT, MODE, TWT>(tile, im, gp, r, src, dst, tw, scale_br, tid, tw_base, !kStageFold, !select); break;
            case 3: run_round<DIF, 3, EPT, MODE, TWT>(tile, im, gp, r, src, dst, tw, scale_br, tid, tw_base, !kStageFold, !select); break;
            default: run_round<DIF, 4, EPT, MODE, TWT>(tile, im, gp, r, src, dst, tw, scale_br, tid, tw_base, !kStageFold, !select); break;
        }
        if (r + 1 < gp.n_rounds) __syncthreads();  // the next round reads what this round wrote
    }
    if (select) {
        // the tile stays in LDS (the forward network's [0, 2p) representatives): this tile's term of every selected output
        __syncthreads();
        const size_t t = blockIdx.x;  // (one tile per workgroup: the host only selects then)
        uint32_t* part = gp.sel_part ? gp.sel_part + ((size_t)blockIdx.y * gp.n_tiles + t) * (size_t)gp.n_sel : nullptr;
        for (int q = tid; q < gp.n_sel; q += kBlock) {
            const uint32_t v = bb::reduce_2p(tile[lds_phys(gp.sel_pos[q])]);
            const uint32_t term = bb::mul(v, gp.sel_xpow[(size_t)q * gp.n_tiles + t]);
            if (part) part[q] = term;  // n_sel consecutive words per workgroup
            else atomicAdd(gp.sel_acc + (size_t)blockIdx.y * gp.n_sel + q, (unsigned long long)term);
        }
    }
}

// all rounds of one stage group on the workgroup's tile(s). TWT: `tw` is the group's twiddle TABLE (FusedTwiddles).
template <bool DIF, int EPT, bool TWT = false>
__device__ __forceinline__ void run_group(uint32_t* tile, const IndexMap& im, const GroupParams& gp, const uint32_t* __restrict__ src,
                                          uint32_t* __restrict__ dst, const uint32_t* __restrict__ tw, int tid, bool io_first, bool io_last) {
    uint32_t tw_base = TWT ? 0u : load_twiddle_base<DIF>(im, gp, 0, 0, tid, tw);
    for (int r = 0; r < gp.n_rounds; ++r) {
        switch (gp.logr[r]) {
            case 1: run_round<DIF, 1, EPT, 0, TWT>(tile, im, gp, r, src, dst, tw, nullptr, tid, tw_base, io_first, io_last); break;
            case 2: run_round<DIF, 2, EPT, 0, TWT>(tile, im, gp, r, src, dst, tw, nullptr, tid, tw_base, io_first, io_last); break;
            case 3: run_round<DIF, 3, EPT, 0, TWT>(tile, im, gp, r, src, dst, tw, nullptr, tid, tw_base, io_first, io_last); break;
            default: run_round<DIF, 4, EPT, 0, TWT>(tile, im, gp, r, src, dst, tw, nullptr, tid, tw_base, io_first, io_last); break;
        }
        if (r + 1 < gp.n_rounds) __syncthreads();
    }
}

// The middle of the LDE in ONE pass over HBM: the last (contiguous) stage group of the inverse transform, the coset
// scaling s^k / H, the zero-padding to 2H (a duplication in bit-reversed order) and the first (contiguous) stage group of
// the forward transform all act on the same 2^ka bit-reversed coefficients, so a workgroup loads them once, runs the DIF
// rounds, expands through LDS and runs the DIT rounds on the 2^(ka+1) results: the H-sized coefficient array is neither
// written nor re-read (8 of the 44 bytes the unfused schedule moves per trace cell). For H <= 2^12 the whole LDE of a
// column is this one launch.
__global__ __launch_bounds__(kBlock) void lde_fused_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t in_stride,
                                                           size_t out_stride, GroupParams ga, GroupParams gd,
                                                           const uint32_t* __restrict__ tw_inv, const uint32_t* __restrict__ tw_fwd,
                                                           const uint32_t* __restrict__ scale_br) {
    constexpr int LOGA = 12, LOGD = 13;
    __shared__ uint32_t tile[(1 << LOGD) + ((1 << LOGD) >> 5)];
    const int tid = threadIdx.x;
    const uint32_t* src = in + (size_t)blockIdx.y * in_stride;
    uint32_t* dst = out + (size_t)blockIdx.y * out_stride;
    IndexMap ia;
    ia.B = ga.B; ia.c = ga.c; ia.lowbits = ga.lowbits; ia.k = ga.k;
    ia.cmask = (1u << ga.c) - 1u;
    ia.tile0 = (size_t)blockIdx.x << (LOGA - ga.B);
    ia.n_tiles = (size_t)ga.n_tiles;
    run_group<true, (1 << LOGA) / kBlock, true>(tile, ia, ga, src, nullptr, tw_inv, tid, true, false);
    __syncthreads();
    // scale and duplicate: element l of the coefficient tile becomes elements 2l, 2l + 1 of the forward tile
    uint32_t v[(1 << LOGA) / kBlock];
#pragma unroll
    for (int m = 0; m < (1 << LOGA) / kBlock; ++m) {
        const uint32_t l = (uint32_t)tid + 256u * m;
        bool valid;
        const size_t q = ia.global(l, valid);
        const uint32_t sc = valid ? scale_br[q] : 0u;
        v[m] = bb::mul(tile[lds_phys(l)], sc);
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < (1 << LOGA) / kBlock; ++m) {
        const uint32_t l = (uint32_t)tid + 256u * m;
        tile[lds_phys(2 * l)] = v[m];
        tile[lds_phys(2 * l + 1)] = v[m];
    }
    __syncthreads();
    IndexMap id;
    id.B = gd.B; id.c = gd.c; id.lowbits = gd.lowbits; id.k = gd.k;
    id.cmask = (1u << gd.c) - 1u;
    id.tile0 = (size_t)blockIdx.x << (LOGD - gd.B);
    id.n_tiles = (size_t)gd.n_tiles;
    run_group<false, (1 << LOGD) / kBlock, true>(tile, id, gd, nullptr, dst, tw_fwd, tid, false, true);
}

// The fused kernel specialised for its one geometry from 2^12 rows up (ka = 12: a 4 096-coefficient tile, 8 192 results, three radix-16
// rounds each way, one passive bit on the forward side), every window, slot count, LDS offset and table offset a constant:
//   A  DIF window 8-11: HBM -> registers -> LDS            (twiddles: per-lane table loads)
//   B  DIF window 4-7:  LDS -> LDS                         (per-lane table loads, requested during A)
//   C  DIF window 0-3:  LDS -> registers                   (15 wave-uniform twiddles)
//   D  DIT window 1-4, both duplicates: registers -> LDS   (2 x 15 wave-uniform twiddles; its first stage multiplies by 1 / H)
//   E  DIT window 5-8:  LDS -> LDS, two slots              (ONE set of per-lane twiddles for both slots, requested during C)
//   F  DIT window 9-12: LDS -> HBM, two slots              (per-lane table loads, requested during E)
// No scale-and-duplicate pass: lane t ends C holding coefficients 16 t .. 16 t + 15 of the tile, and the two slots of D whose inputs
// are their duplicates — positions 32 t + 2 rho + b of the doubled tile, b = the passive bit — are the slots 2 t and 2 t + 1, so the
// lane runs both from its registers (one set of inputs, two sets of twiddles). The coset factor s^k is in the forward twiddles (stage
// s of the size-2^(n+1) transform carries s^(2^(n-s)): the table is built per height, fused12_twiddles, and the strided DIT groups
// multiply their round bases by GroupParams::cst); 1 / H is in the constants of D's first stage.
// A, B, C run the unsigned butterflies of slot_butterflies on canonical words; D, E, F the signed ones below (ntt::bounds), and F's
// store returns to canonical words.
// Per tile: 5 barriers (the generic kernel: 7), 24 576 LDS words written and 24 576 read (36 864 each).
// Barrier 3 (between C and D): positions 32 t .. 32 t + 31 of the doubled tile are other lanes' coefficients 16 t .. 16 t + 15 of
// the single one, so every lane must have read its C slot before any lane writes a D result.
// LDS layout: lds_phys (one pad word per 32), 32-bit accesses, every one conflict-free per half-wave (32 banks): A / E / F move 32
// consecutive words; B two runs of 16 words 528 = 16 (mod 32) words apart (see there); C reads with a lane stride of 16.5 words (banks
// 16 (t & 1) + (t >> 1)) and D writes with one of 33 words. (The generic kernel's window 4-7 round is 2-way conflicting: measured.)
constexpr uint32_t kF12A0 = 0, kF12A1 = 15u * 256u, kF12A2 = kF12A1 + 15u * 16u;   // DIF tables: windows 8-11, 4-7, 0-3
constexpr uint32_t kF12D0 = 4096, kF12D1 = kF12D0 + 15u * 2u, kF12D2 = kF12D1 + 15u * 32u;  // DIT tables: windows 1-4, 5-8, 9-12
constexpr uint32_t kF12Words = kF12D2 + 15u * 512u;

template <int RB>
__device__ constexpr uint32_t f12_off(int rho) {
    return ((uint32_t)rho << RB) + (RB >= 5 ? ((uint32_t)rho << (RB >= 5 ? RB - 5 : 0)) : ((uint32_t)rho >> (RB >= 5 ? 0 : 5 - RB)));
}

// The forward rounds D, E, F run on SIGNED representatives (bb::dit_signed): the ranges they rely on, as exact integers. D's inputs are
// the canonical words C leaves; the forward tables hold centred twiddles (fused12_twiddles) and kappa is R mod p or, in D's first stage,
// the centred word of 1 / H; every butterfly
// maps magnitudes below kInTop to magnitudes below kOutTop <= kInTop, so three rounds of four stages need no correction in between,
// and F's store makes its words canonical with bb::canonical_of_centred. tests/test_ntt_signed_bounds.py recomputes every figure and
// presents the edges to the host path of bb::dit_signed. p = 2013265921.
namespace ntt {
namespace bounds {
constexpr int64_t kSmontDomain = 4899916392431616000ll;  // 2^63 - 2^31 p = 1.209 p^2: bb::smont takes |t| < this
constexpr int64_t kInTop = 2013265921ll;                  // p (B = 1): |a|, |b| < this; canonical words are inside
constexpr int64_t kTwiddleTop = 1006632960ll;             // (p - 1) / 2: |w|, |kappa| <= this
constexpr int64_t kWideTop = 4053239664633446400ll;       // 2 (kInTop - 1) kTwiddleTop = (p - 1)^2 = 1.000 p^2: |a kappa + b w| <= this
constexpr int64_t kOutTop = 1950351361ll;                 // floor((kWideTop + 2^31 p) / 2^32) + 1 = 0.96875 p: |output| < this
static_assert(kSmontDomain == (int64_t)((1ull << 63) - ((uint64_t)bb::P << 31)), "smont's domain");
static_assert(kInTop == (int64_t)bb::P && kTwiddleTop == (int64_t)(bb::P - 1) / 2, "B = 1, centred twiddles");
static_assert(kWideTop == 2 * (kInTop - 1) * kTwiddleTop && kWideTop < kSmontDomain, "a kappa + b w stays inside smont's domain");
static_assert(kOutTop == (int64_t)(((uint64_t)kWideTop + ((uint64_t)bb::P << 31)) >> 32) + 1, "the reduction adds at most 2^31 p");
static_assert(kOutTop <= kInTop, "the range closes: outputs are inputs of the next stage");
static_assert(kOutTop + (int64_t)bb::P <= (1ll << 32), "canonical_of_centred: x + p does not wrap for x >= 0");
static_assert((int64_t)bb::R_MOD_P <= kTwiddleTop, "kappa = R mod p is centred as it stands");
}  // namespace bounds
}  // namespace ntt

// One radix-16 slot of a forward round on signed representatives: `tt` as slot_butterflies' table form, centred; kappa0: the factor of
// `a` in the slot's first stage (R mod p, or a constant the stage multiplies by: its twiddles then carry the same constant).
// -w is one full-rate negation per twiddle, 15 per slot (E's two slots share theirs; D's twiddles are wave-uniform: none). Measured
// against -b per butterfly (the compiler negates the 64-bit product instead: 2 instructions) and against a second, negated table
// (15 more loads and registers per slot, 132 VGPRs): 1.35 against 1.39 and 1.40 ms at 256 x 2^20 (profiles/lde_fused_signed.txt).
__device__ __forceinline__ void slot_dit_signed(int32_t* v, const int32_t* tt, int32_t kappa0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int lowp = u & ((1 << q) - 1);
            const int i0 = ((u >> q) << (q + 1)) | lowp;
            const int i1 = i0 | (1 << q);
            const int32_t w = tt[(1 << q) - 1 + lowp];
            bb::dit_signed(v[i0], v[i1], w, -w, q == 0 ? kappa0 : (int32_t)bb::R_MOD_P);
        }
    }
}

// hinv_c: the centred representative of the Montgomery word of 1 / H (D's first stage: see there)
__global__ __launch_bounds__(kBlock) void lde_fused12_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t in_stride,
                                                             size_t out_stride, const uint32_t* __restrict__ tw, int32_t hinv_c) {
    __shared__ uint32_t tile[(1 << 13) + ((1 << 13) >> 5)];
    const uint32_t tid = threadIdx.x;
    const uint32_t* src = in + (size_t)blockIdx.y * in_stride + ((size_t)blockIdx.x << 12);
    uint32_t* dst = out + (size_t)blockIdx.y * out_stride + ((size_t)blockIdx.x << 13);
    uint32_t x[16], tt[16], tn[16];
    int32_t te[16];
    // ---- A ----
#pragma unroll
    for (int rho = 0; rho < 16; ++rho) x[rho] = src[tid + 256u * rho];
#pragma unroll
    for (int j = 0; j < 15; ++j) tt[j] = tw[kF12A0 + 256u * j + tid];
#pragma unroll
    for (int j = 0; j < 15; ++j) tn[j] = tw[kF12A1 + 16u * j + (tid & 15u)];
    slot_butterflies<true, 4, true>(x, 0u, tt);
    {
        const uint32_t p0 = lds_phys(tid);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) tile[p0 + f12_off<8>(rho)] = x[rho];
    }
    __syncthreads();
    // ---- B ----
    {
        // slot = (k, low), elements 256 k + 16 rho + low; low = lane bits 0-3, and k takes lane bits 4 and 5 SWAPPED: a half-wave
        // then holds k0 and k0 + 2, whose runs of 16 words lie 528 = 16 (mod 32) words apart (k0, k0 + 1: 264 = 8, a 2-way conflict)
        const uint32_t k = ((tid >> 5) & 1u) | (((tid >> 4) & 1u) << 1) | ((tid >> 6) << 2);
        const uint32_t p0 = lds_phys((k << 8) | (tid & 15u));
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) x[rho] = tile[p0 + f12_off<4>(rho)];
        slot_butterflies<true, 4, true>(x, 0u, tn);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) tile[p0 + f12_off<4>(rho)] = x[rho];
    }
    __syncthreads();
    // ---- C ----
    {
        const uint32_t p0 = lds_phys(tid << 4);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) x[rho] = tile[p0 + (uint32_t)rho];
#pragma unroll
        for (int j = 0; j < 15; ++j) te[j] = (int32_t)tw[kF12D1 + 32u * j + (tid & 31u)];  // for E
#pragma unroll
        for (int j = 0; j < 15; ++j) tt[j] = tw[kF12A2 + j];
        slot_butterflies<true, 4, true>(x, 0u, tt);
    }
    __syncthreads();
    // ---- D ---- (from here on signed representatives: ntt::bounds; the inputs are C's canonical words)
    // 1 / H rides in the first stage: a kappa + b w with kappa = (1 / H) R and the stage's twiddles times 1 / H (fused12_twiddles)
    // gives (a + b w) / H and (a - b w) / H — no product per coefficient.
    {
        const uint32_t p0 = lds_phys(tid << 5);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            int32_t y[16], ts[16];
#pragma unroll
            for (int rho = 0; rho < 16; ++rho) y[rho] = (int32_t)x[rho];
#pragma unroll
            for (int j = 0; j < 15; ++j) ts[j] = (int32_t)tw[kF12D0 + 2u * j + b];
            slot_dit_signed(y, ts, hinv_c);
#pragma unroll
            for (int rho = 0; rho < 16; ++rho) tile[p0 + 2u * rho + b] = (uint32_t)y[rho];
        }
    }
    __syncthreads();
    // ---- E ----
    int32_t tf[2][16], sx[16];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int j = 0; j < 15; ++j) tf[m][j] = (int32_t)tw[kF12D2 + 512u * j + tid + 256u * m];  // for F
    }
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const uint32_t sigma = tid + 256u * m;
        const uint32_t p0 = lds_phys(((sigma >> 5) << 9) | (sigma & 31u));
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) sx[rho] = (int32_t)tile[p0 + f12_off<5>(rho)];
        slot_dit_signed(sx, te, (int32_t)bb::R_MOD_P);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) tile[p0 + f12_off<5>(rho)] = (uint32_t)sx[rho];
    }
    __syncthreads();
    // ---- F ---- (its store makes the words canonical: the strided forward groups take [0, 2p), and at 2^12 rows it is the LDE's last)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const uint32_t sigma = tid + 256u * m;
        const uint32_t p0 = lds_phys(sigma);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) sx[rho] = (int32_t)tile[p0 + f12_off<9>(rho)];
        slot_dit_signed(sx, tf[m], (int32_t)bb::R_MOD_P);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) dst[sigma + 512u * rho] = bb::canonical_of_centred(sx[rho]);
    }
}

// The strided stage group of the fused schedule at 2^20 rows (K = 8 stages: stages 0-7 of the size-2^20 inverse transform into `tmp`,
// stages 13-20 of the size-2^21 forward one in place on `out`) with its geometry as constants — what ntt_group_kernel<DIF, 13, 0> does
// for the group make_group(DIF, DIF ? 20 : 21, DIF ? 0 : 13, 8, 5), word for word: a 2^13-element tile of 256 rows of 32 consecutive
// words (c = 5: 128-byte segments), LB = log2 of the word distance between two rows (the group's `lowbits`), tile t of a column at
// word 32 t. Two radix-16 rounds, two slots per lane and round:
//   "hi", window 9-12: slot (tid, m) holds rows (tid >> 5) + 8 m + 16 rho, column tid & 31
//   "lo", window 5-8:  slot (tid, m) holds rows 16 ((tid >> 5) + 8 m) + rho, column tid & 31
// DIF runs hi then lo, DIT lo then hi; the first round loads from HBM, the second stores to it, LDS (lds_phys) in between.
// Straight-line code: the tile and twiddle positions are wave-uniform bases (scalar registers) plus ONE 32-bit byte offset per lane
// and round kind, the per-element strides constants on the scalar side; a lane issues all 32 loads of its two slots and its three
// twiddle bases (one per hi slot; the lo slots of a lane share theirs: it depends on the column only) before the first butterfly.
// cst_lo / cst_hi: the coset constants of the two rounds' top stages (GroupParams::cst; the Montgomery one without a coset: a product
// that returns its canonical argument). The forward group reduces to [0, p) on its store (it is the transform's last).
// A workgroup reads and writes its own tile's positions only, so the forward group is safe in place.
template <int RB>
__device__ __forceinline__ constexpr uint32_t strided8_words(int lb, int m, int rho) {  // slot m, element rho: words from the lane's base
    return RB == 9 ? (((uint32_t)(8 * m) << lb) + ((uint32_t)rho << (lb + 4))) : (((uint32_t)m << (lb + 7)) + ((uint32_t)rho << lb));
}
// base + off4 bytes as the global access with a scalar base and a 32-bit lane offset (pwj::ld's form). `base` — wave-uniform, a constant
// stride already added — passes through an empty asm statement that pins it to a scalar register pair: left to itself the compiler
// moves the constant into a 64-bit lane addition per access (two VALU instructions each, 128 per wave).
// (The pointers are named global ones: behind the asm statement the compiler no longer sees where they came from.)
typedef __attribute__((address_space(1))) const char* GlobalBytesIn;
typedef __attribute__((address_space(1))) char* GlobalBytesOut;
__device__ __forceinline__ uint32_t ld_off4(const uint32_t* base, uint32_t off4) {
    GlobalBytesIn b = (GlobalBytesIn)base;
    asm("" : "+s"(b));
    return *(__attribute__((address_space(1))) const uint32_t*)(b + off4);
}
__device__ __forceinline__ void st_off4(uint32_t* base, uint32_t off4, uint32_t v) {
    GlobalBytesOut b = (GlobalBytesOut)base;
    asm("" : "+s"(b));
    *(__attribute__((address_space(1))) uint32_t*)(b + off4) = v;
}

template <bool DIF, int K>
__global__ __launch_bounds__(kBlock) void ntt_strided_kernel(const uint32_t* in, uint32_t* out, size_t in_stride, size_t out_stride,
                                                             const uint32_t* __restrict__ tw, uint32_t cst_lo, uint32_t cst_hi) {
    static_assert(K == 8, "the 2^20-row geometry; other heights take ntt_group_kernel");
    constexpr int LB = DIF ? 12 : 13;
    constexpr int RB0 = DIF ? 9 : 5, RB1 = DIF ? 5 : 9;  // the two rounds' windows, in execution order
    __shared__ uint32_t tile[(1 << 13) + ((1 << 13) >> 5)];
    const uint32_t tid = threadIdx.x, row = tid >> 5, col = tid & 31u;
    const size_t t0 = (size_t)blockIdx.x << 5;
    const uint32_t* src = in + (size_t)blockIdx.y * in_stride + t0;
    uint32_t* dst = out + (size_t)blockIdx.y * out_stride + t0;
    const uint32_t off_hi = 4u * ((row << LB) | col), off_lo = 4u * ((row << (LB + 4)) | col);  // byte offsets of the lane's slot 0
    const uint32_t off0 = RB0 == 9 ? off_hi : off_lo, off1 = RB1 == 9 ? off_hi : off_lo;
    // ---- every load of the tile, then the twiddle bases ----
    uint32_t x[2][16];
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) x[m][rho] = ld_off4(src + strided8_words<RB0>(LB, m, rho), off0);
    }
    // hi: w^g, g = the slot's row and column and the tile (its global index below the window); lo: w^(16 g), g = tile and column
    uint32_t b_hi[2], b_lo;
#pragma unroll
    for (int m = 0; m < 2; ++m) b_hi[m] = ld_off4(tw + t0 + ((uint32_t)(8 * m) << LB), off_hi);
    b_lo = ld_off4(tw + (t0 << 4), col << 6);
    if (!DIF) {
        b_lo = bb::mul(b_lo, cst_lo);
#pragma unroll
        for (int m = 0; m < 2; ++m) b_hi[m] = bb::mul(b_hi[m], cst_hi);
    }
    // padded LDS positions of the lane's slot 0; slot 1 lies 264 (hi) / 4 224 (lo) words further
    const uint32_t p_hi = lds_phys(tid), p_lo = (row << 9) + (row << 4) + col;
    const uint32_t p0 = RB0 == 9 ? p_hi : p_lo, p1 = RB1 == 9 ? p_hi : p_lo;
    constexpr uint32_t kSlot0 = RB0 == 9 ? 264u : 4224u, kSlot1 = RB1 == 9 ? 264u : 4224u;
    // ---- first round: registers -> LDS ----
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        slot_butterflies<DIF, 4>(x[m], RB0 == 9 ? b_hi[m] : b_lo);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) tile[p0 + kSlot0 * m + f12_off<RB0>(rho)] = x[m][rho];
    }
    __syncthreads();
    // ---- second round: LDS -> HBM ----
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        uint32_t y[16];
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) y[rho] = tile[p1 + kSlot1 * m + f12_off<RB1>(rho)];
        slot_butterflies<DIF, 4>(y, RB1 == 9 ? b_hi[m] : b_lo);
#pragma unroll
        for (int rho = 0; rho < 16; ++rho) st_off4(dst + strided8_words<RB1>(LB, m, rho), off1, DIF ? y[rho] : bb::reduce_2p(y[rho]));
    }
}

struct Tables {
    uint32_t* tw_fwd = nullptr;    // g_n^j, j < 2^(n-1)
    uint32_t* tw_inv = nullptr;    // g_n^-j
    uint32_t* shift = nullptr;     // s^k / 2^n, k < 2^n
    uint32_t* shift_br = nullptr;  // shift[bitrev_n(q)]
};
std::mutex g_mu;
std::map<std::pair<int, int>, Tables> g_tables;  // (device, n): twiddle tables live on the device that was current when they were built
uint64_t g_roots_uploaded = 0;                   // bit d: device d's __constant__ copy of the 16th roots is initialised

int upload_roots() {
    int device = 0;
    PW_HIP_TRY(hipGetDevice(&device));
    if (device < 64 && (g_roots_uploaded >> device) & 1) return 0;
    uint32_t h[2][8];
    const uint32_t w16 = field::root_of_unity(4), w16i = bb::inv(w16);
    uint32_t a = bb::R_MOD_P, b = bb::R_MOD_P;
    for (int r = 0; r < 8; ++r) { h[0][r] = a; h[1][r] = b; a = bb::mul(a, w16); b = bb::mul(b, w16i); }
    PW_HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_roots16), h, sizeof h));
    if (device < 64) g_roots_uploaded |= 1ull << device;
    return 0;
}

const Tables* tables(int n) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (upload_roots()) return nullptr;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return nullptr;
    const std::pair<int, int> key{device, n};
    auto it = g_tables.find(key);
    if (it != g_tables.end()) return &it->second;
    Tables t;
    size_t half = n ? (size_t)1 << (n - 1) : 1, full = (size_t)1 << n;
    if (hipMalloc(&t.tw_fwd, half * 4) != hipSuccess) return nullptr;
    if (hipMalloc(&t.tw_inv, half * 4) != hipSuccess) return nullptr;
    if (hipMalloc(&t.shift, full * 4) != hipSuccess) return nullptr;
    if (hipMalloc(&t.shift_br, full * 4) != hipSuccess) return nullptr;
    uint32_t w = field::root_of_unity(n);
    uint32_t one = bb::R_MOD_P;
    hipLaunchKernelGGL(fill_powers_kernel, dim3(div_up(half, 256)), dim3(256), 0, stream(), t.tw_fwd, w, one, half);
    hipLaunchKernelGGL(fill_powers_kernel, dim3(div_up(half, 256)), dim3(256), 0, stream(), t.tw_inv, bb::inv(w), one, half);
    uint32_t ninv = bb::inv(bb::to_monty((uint32_t)(((uint64_t)1 << n) % bb::P)));
    hipLaunchKernelGGL(fill_powers_kernel, dim3(div_up(full, 256)), dim3(256), 0, stream(), t.shift,
                       bb::to_monty(field::kCosetShift), ninv, full);
    hipLaunchKernelGGL(bitrev_copy_kernel, dim3(div_up(full, 256)), dim3(256), 0, stream(), t.shift, t.shift_br, n);
    // other host threads (other streams) may use the tables as soon as they are published
    if (hipStreamSynchronize(stream()) != hipSuccess) return nullptr;
    return &g_tables.emplace(key, t).first->second;
}

// Stages [s, s + k) of a size-2^n transform as one group on tiles that carry c passive low bits, cut into rounds
GroupParams make_group(bool dif, int n, int s, int k, int c) {
    GroupParams g{};
    g.n = n; g.s0 = s; g.k = k; g.c = c; g.lowbits = dif ? n - s - k : s; g.B = k + c;
    g.n_tiles = 1ull << (n - g.B);
    // rounds: ceil(k/4) windows of nearly equal width
    int nr = (k + 3) / 4;
    g.n_rounds = nr;
    int widths[4];
    for (int r = 0; r < nr; ++r) widths[r] = k / nr + (r < k % nr ? 1 : 0);
    if (dif) {  // from the top active bit downwards
        int top = c + k;
        for (int r = 0; r < nr; ++r) { top -= widths[r]; g.rb[r] = top; g.logr[r] = widths[r]; }
    } else {    // from the lowest active bit upwards
        int bot = c;
        for (int r = 0; r < nr; ++r) { g.rb[r] = bot; g.logr[r] = widths[r]; bot += widths[r]; }
    }
    return g;
}

// Split stages [first, n) into groups of at most `LOGT - c` stages, every group on tiles of 2^logt_out elements.
// `end` < n: only the stages [first, end) (the fused LDE kernel takes the rest); `balance`: the groups get nearly equal numbers
// of stages instead of greedy-full groups followed by a short one.
std::vector<GroupParams> plan_groups(bool dif, int n, int first, int& logt_out, int end = -1, bool balance = false) {
    std::vector<GroupParams> out;
    // 2^c neighbouring elements ride along in strided tiles: 64-byte segments (c = 4) up to 2^17 rows, 128-byte ones (c = 5) from
    // 2^18 rows on, where the strided passes run at 3.5 TB/s with 64-byte segments (profiles/r02_bench_ntt.txt); POWDR_NTT_C forces one
    int kStridedC = (n - (dif ? 0 : 1)) >= 18 ? 5 : 4;  // n = log2 of the transform: the LDE's forward half has one bit more
    if (const char* e = getenv("POWDR_NTT_C")) { int v = atoi(e); if (v >= 0 && v <= 6) kStridedC = v; }
    if (end < 0) end = n;
    const int total = end - first;
    // tile size: 2^13 when it saves a pass or the transform is large, else 2^12
    int logt = 12;
    int n_groups = 0;
    {
        auto passes = [&](int lt) {
            int s = first, p = 0;
            while (s < end) {
                int rem = end - s, k = rem < lt ? rem : lt;
                for (; k >= 1; --k) { int lb = dif ? n - s - k : s; int c = lb < kStridedC ? lb : kStridedC; if (k + c <= lt) break; }
                s += k; ++p;
            }
            return p;
        };
        if (total > 0 && passes(13) < passes(12)) logt = 13;
        n_groups = total > 0 ? passes(logt) : 0;
    }
    logt_out = logt;
    int s = first;
    int groups_left = n_groups;
    while (s < end) {
        int rem = end - s, k = rem < logt ? rem : logt;
        if (balance && groups_left > 0) { const int target = (rem + groups_left - 1) / groups_left; if (k > target) k = target; }
        --groups_left;
        int c = 0;
        for (; k >= 1; --k) { int lb = dif ? n - s - k : s; c = lb < kStridedC ? lb : kStridedC; if (k + c <= logt) break; }
        out.push_back(make_group(dif, n, s, k, c));
        s += k;
    }
    return out;
}

// Twiddle table of ONE tile-invariant stage group (lowbits == c: the group's factors depend on the tile-local index only —
// the last stages of an inverse / the first stages of a forward transform). Per round [stage-major twiddle index j <
// 2^logr - 1][g < 2^rb]: the roots of order 2^(rb + logr) to the power g, times the constant 2^(q+1)-th roots of the stage.
void append_group_table(std::vector<uint32_t>& h, const GroupParams& gp, bool dif, unsigned* offs, size_t base) {
    const uint32_t w16 = field::root_of_unity(4), w16i = bb::inv(w16);
    uint32_t roots[8];
    { uint32_t a = bb::R_MOD_P; for (int r = 0; r < 8; ++r) { roots[r] = a; a = bb::mul(a, dif ? w16i : w16); } }
    for (int r = 0; r < gp.n_rounds; ++r) {
        const int rb = gp.rb[r], logr = gp.logr[r];
        offs[r] = (unsigned)(h.size() - base);
        const size_t G = (size_t)1 << rb, J = ((size_t)1 << logr) - 1;
        h.resize(h.size() + J * G);
        uint32_t* tab = h.data() + base + offs[r];
        uint32_t om = field::root_of_unity(rb + logr);
        if (dif) om = bb::inv(om);
        uint32_t bt = bb::R_MOD_P;  // om^g
        for (size_t g = 0; g < G; ++g) {
            uint32_t bq[4];
            bq[logr - 1] = bt;
            for (int q = logr - 2; q >= 0; --q) bq[q] = bb::sqr(bq[q + 1]);
            for (int q = 0; q < logr; ++q)
                for (int rr = 0; rr < (1 << q); ++rr)
                    tab[(((size_t)1 << q) - 1 + rr) * G + g] = rr == 0 ? bq[q] : bb::mul(bq[q], roots[rr << (3 - q)]);
            bt = bb::mul(bt, om);
        }
    }
}

// The twiddle caches below: cache[(device, key)], an Entry whose `d` is a device table that lives as long as the process. A missing
// entry is built on the host (build(words, entry): false = no table), uploaded synchronously — it is published complete: other host
// threads, on other streams, may use it at once — and kept. nullptr: no table (nothing is kept, and nothing stays allocated).
template <class Key, class Entry, class Build>
const Entry* cached_table(std::map<std::pair<int, Key>, Entry>& cache, const Key& key, Build&& build) {
    std::lock_guard<std::mutex> lk(g_mu);
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) return nullptr;
    const std::pair<int, Key> dk{device, key};
    auto it = cache.find(dk);
    if (it != cache.end()) return &it->second;
    Entry e;
    std::vector<uint32_t> h;
    if (!build(h, e) || h.empty()) return nullptr;
    if (hipMalloc(&e.d, h.size() * 4) != hipSuccess) return nullptr;
    if (hipMemcpy(e.d, h.data(), h.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(e.d); return nullptr; }
    return &cache.emplace(dk, e).first->second;
}

struct GroupTwiddles { uint32_t* d = nullptr; unsigned off[4] = {0, 0, 0, 0}; };
std::map<std::pair<int, std::tuple<int, int, int>>, GroupTwiddles> g_group_tw;  // (device, (dif, c, k))
// nullptr: the group is not tile-invariant (or the table could not be built): the kernel derives its twiddles
const GroupTwiddles* group_twiddles(const GroupParams& gp, bool dif) {
    if (gp.lowbits != gp.c) return nullptr;
    return cached_table(g_group_tw, std::make_tuple(dif ? 1 : 0, gp.c, gp.k), [&](std::vector<uint32_t>& h, GroupTwiddles& gt) {
        append_group_table(h, gp, dif, gt.off, 0);
        return true;
    });
}

// A tile-invariant group's twiddle table with a sub-coset's constants folded in: entry (round r, stage q of the round) times cq[r][q]
struct CosetTableArgs { unsigned off[4]; int rb[4], logr[4]; int n_rounds; uint32_t cq[4][4]; unsigned total; };
__global__ void coset_table_kernel(const uint32_t* __restrict__ tab, uint32_t* __restrict__ out, CosetTableArgs a) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    int r = 0;
    while (r + 1 < a.n_rounds && i >= a.off[r + 1]) ++r;
    const unsigned j = (i - a.off[r]) >> a.rb[r];  // stage-major twiddle index: stage q holds j in [2^q - 1, 2^(q+1) - 1)
    const int q = 31 - __clz((int)(j + 1));
    out[i] = bb::mul(tab[i], a.cq[r][q]);
}

// Sub-coset evaluation (subcoset_lde): the first group loads with FOLD, every stage's twiddles carry the coset constant C[stage]
struct CosetSpec {
    int fold_log;
    uint32_t foldk[16];
    uint32_t C[32];       // C[s] = c^(2^(n-1-s)), s < n
    uint32_t* d_scratch;  // room for a group's derived twiddle table (< 2^13 words)
    // SELECT (GroupParams): only with max_groups = 1 and one tile per workgroup
    int n_sel = 0;
    const uint32_t* sel_pos = nullptr;
    const uint32_t* sel_xpow = nullptr;
    unsigned long long* sel_acc = nullptr;
    uint32_t* sel_part = nullptr;
};

// blockIdx.y is the column and a grid has at most 65 535 of them: launch(c0, cc) for the chunks [c0, c0 + cc) of `cols` columns
template <class Launch>
void for_column_chunks(uint32_t cols, Launch&& launch) {
    for (uint32_t c0 = 0; c0 < cols; c0 += 65535u) launch(c0, cols - c0 < 65535u ? cols - c0 : 65535u);
}

// ntt_group_kernel<DIF, logt, mode, table != nullptr> (the twiddle argument: `table`, else the transform's roots `tw`). EXPAND and
// FOLD loads exist in the forward direction only.
template <bool DIF>
void launch_group_kernel(int logt, int mode, dim3 grid, const uint32_t* src, uint32_t* dst, size_t src_stride, size_t dst_stride,
                         const GroupParams& g, const uint32_t* table, const uint32_t* tw, const uint32_t* scale_br) {
    auto launch = [&](auto lt, auto md) {
        constexpr int LT = decltype(lt)::value, MD = decltype(md)::value;
        if (table) hipLaunchKernelGGL((ntt_group_kernel<DIF, LT, MD, true>), grid, dim3(kBlock), 0, stream(), src, dst, src_stride, dst_stride, g, table, scale_br);
        else hipLaunchKernelGGL((ntt_group_kernel<DIF, LT, MD, false>), grid, dim3(kBlock), 0, stream(), src, dst, src_stride, dst_stride, g, tw, scale_br);
    };
    auto with_mode = [&](auto lt) {
        if constexpr (!DIF) {
            if (mode == 2) return launch(lt, std::integral_constant<int, 2>{});
            if (mode == 1) return launch(lt, std::integral_constant<int, 1>{});
        }
        launch(lt, std::integral_constant<int, 0>{});
    };
    if (logt == 13) with_mode(std::integral_constant<int, 13>{});
    else with_mode(std::integral_constant<int, 12>{});
}

// Is `g` on 2^logt tiles the group ntt_strided_kernel<DIF, 8> is written for? (The kernel's constants restate what make_group derives.)
template <bool DIF>
bool strided8_geometry(const GroupParams& g, int logt) {
    return logt == 13 && g.n == (DIF ? 20 : 21) && g.s0 == (DIF ? 0 : 13) && g.k == 8 && g.c == 5 && g.lowbits == (DIF ? 12 : 13) && g.B == 13 &&
           g.n_tiles == (DIF ? 128ull : 256ull) && g.n_rounds == 2 && g.logr[0] == 4 && g.logr[1] == 4 && g.rb[0] == (DIF ? 9 : 5) &&
           g.rb[1] == (DIF ? 5 : 9) && (DIF || g.canonical_out) && !g.fold && !g.n_sel;
}

// The groups of a plan, one launch per group and column chunk, on tiles of 2^logt elements: the first from `in` with the loads of
// `mode` (ntt_group_kernel: 1 = EXPAND with `expand_scale_br`, 2 = FOLD with cs), the others in place on `out` with plain loads.
// Tile-invariant groups read their twiddles from a table. cs: a sub-coset transform (FOLD / SELECT, the coset's constants in every
// group's twiddles). coset_pw (the LDE behind lde_fused12_kernel): pw[e] = s^(2^e); the twiddles of stage s carry s^(2^(n-1-s)).
template <bool DIF>
void launch_groups(std::vector<GroupParams>& groups, int logt, int mode, const uint32_t* in, uint32_t* out, size_t in_stride, size_t out_stride,
                   uint32_t cols, const uint32_t* tw, const uint32_t* expand_scale_br, const char* name, const CosetSpec* cs = nullptr,
                   const uint32_t* coset_pw = nullptr, bool fused_schedule = false) {
    const uint32_t* src = in;
    size_t src_stride = in_stride;
    for (auto& g : groups) {
        const unsigned wgs = (unsigned)div_up((size_t)g.n_tiles, (size_t)1 << (logt - g.B));
        const GroupTwiddles* gt = group_twiddles(g, DIF);
        if (gt) for (int r = 0; r < 4; ++r) g.twt_off[r] = gt->off[r];
        const uint32_t* table = gt ? gt->d : nullptr;
        if (coset_pw) {
            g.coset = 1;
            for (int r = 0; r < g.n_rounds; ++r) g.cst[r] = coset_pw[g.n - 1 - (g.s0 + g.rb[r] + g.logr[r] - 1 - g.c)];
        }
        if (cs) {
            g.coset = 1;
            g.fold = mode == 2 ? cs->fold_log : 0;
            for (int k = 0; k < 16; ++k) g.foldk[k] = cs->foldk[k];
            if (mode == 2 && cs->n_sel > 0) { g.n_sel = cs->n_sel; g.sel_pos = cs->sel_pos; g.sel_xpow = cs->sel_xpow; g.sel_acc = cs->sel_acc; g.sel_part = cs->sel_part; }
            for (int r = 0; r < g.n_rounds; ++r) g.cst[r] = cs->C[g.s0 + g.rb[r] + g.logr[r] - 1 - g.c];
            if (gt) {
                CosetTableArgs a{};
                a.n_rounds = g.n_rounds;
                for (int r = 0; r < g.n_rounds; ++r) {
                    a.off[r] = gt->off[r]; a.rb[r] = g.rb[r]; a.logr[r] = g.logr[r];
                    for (int q = 0; q < g.logr[r]; ++q) a.cq[r][q] = cs->C[g.s0 + g.rb[r] - g.c + q];
                }
                const int lr = g.n_rounds - 1;
                a.total = gt->off[lr] + (((1u << g.logr[lr]) - 1u) << g.rb[lr]);
                hipLaunchKernelGGL(coset_table_kernel, dim3(div_up(a.total, 256)), dim3(256), 0, stream(), gt->d, cs->d_scratch, a);
                table = cs->d_scratch;
            }
        }
        // the fused schedule's strided group at 2^20 rows: ntt_strided_kernel<DIF, 8> (lde_fused passes fused_schedule unless
        // POWDR_NTT_STRIDED_GENERIC=1); the same timer name, so reports sum the group under one label whichever kernel ran
        if (fused_schedule && mode == 0 && !table && !cs && strided8_geometry<DIF>(g, logt)) {
            const uint32_t one = bb::R_MOD_P;
            const uint32_t cst_lo = g.coset ? g.cst[DIF ? 1 : 0] : one, cst_hi = g.coset ? g.cst[DIF ? 0 : 1] : one;
            for_column_chunks(cols, [&](uint32_t c0, uint32_t cc) {
                ScopedKernelTimer t(name);
                call_stats()[kStatNttStridedFixedLaunches] += 1;
                hipLaunchKernelGGL((ntt_strided_kernel<DIF, 8>), dim3((unsigned)g.n_tiles, cc), dim3(kBlock), 0, stream(), src + (size_t)c0 * src_stride,
                                   out + (size_t)c0 * out_stride, src_stride, out_stride, tw, cst_lo, cst_hi);
            });
            src = out;
            src_stride = out_stride;
            continue;
        }
        for_column_chunks(cols, [&](uint32_t c0, uint32_t cc) {
            // (the sub-coset transforms' first group — FOLD loads, the sub-coset's own twiddle table — has a timer of its own)
            ScopedKernelTimer t(mode == 2 ? "ntt_subcoset_first_group_kernel" : name);
            launch_group_kernel<DIF>(logt, mode, dim3(wgs, cc), src + (size_t)c0 * src_stride, out + (size_t)c0 * out_stride, src_stride, out_stride,
                                     g, table, tw, expand_scale_br);
        });
        src = out;
        src_stride = out_stride;
        mode = 0;
        expand_scale_br = nullptr;
    }
}

// A whole transform (or its stages from `first_stage`): plan and launch
template <bool DIF>
void run_groups(const uint32_t* in, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n,
                int first_stage, const uint32_t* tw, const uint32_t* expand_scale_br, const char* name, const CosetSpec* cs = nullptr,
                int max_groups = -1, int* stages_done = nullptr) {
    int logt = 12;
    auto groups = plan_groups(DIF, n, first_stage, logt);
    // max_groups: only the first groups of the plan (subcoset_lde_first_group: the rest is evaluated for a few outputs only)
    if (max_groups >= 0 && (size_t)max_groups < groups.size()) groups.resize((size_t)max_groups);
    if (stages_done) { *stages_done = first_stage; for (auto& g : groups) *stages_done += g.k; }
    const bool complete = !stages_done || *stages_done == n;
    if (!groups.empty() && complete) groups.back().canonical_out = 1;
    launch_groups<DIF>(groups, logt, cs ? 2 : expand_scale_br != nullptr ? 1 : 0, in, out, in_stride, out_stride, cols, tw, expand_scale_br, name, cs);
    if (groups.empty() && in != out) {
        for (uint32_t c = 0; c < cols; ++c)
            (void)hipMemcpyAsync(out + (size_t)c * out_stride, in + (size_t)c * in_stride, (size_t)4 << n,
                                 hipMemcpyDeviceToDevice, stream());
    }
}

// out[2q] = out[2q+1] = in[q] * scale_br[q]  (only used when the forward transform has no DIT stage
// left after the duplication, i.e. H = 1)
__global__ void expand_small_kernel(const uint32_t* in, uint32_t* out, size_t in_stride, size_t out_stride, size_t h,
                                    const uint32_t* scale_br) {
    size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= h) return;
    uint32_t v = bb::mul(in[(size_t)blockIdx.y * in_stride + q], scale_br[q]);
    out[(size_t)blockIdx.y * out_stride + 2 * q] = v;
    out[(size_t)blockIdx.y * out_stride + 2 * q + 1] = v;
}

// Twiddle tables of the fused kernel's two contiguous groups. In a contiguous group the twiddle of a butterfly depends on
// the tile-local index only — the stages are the last ones of the inverse / the first ones of the forward transform, their
// factors are the roots of order 2^(rb + logr) of a round with window [rb, rb + logr) whatever the transform size — so a
// table per round, [stage-major twiddle index j < 2^logr - 1][g < 2^rb], serves every tile, column and size: <= 46 KB for
// ka = 12, L2-resident, each of a slot's 15 loads one coalesced 256-byte read per wave. Replaces 3 squarings + 11 products
// per radix-16 slot (70 of its 390 instructions).
struct FusedTwiddles {
    uint32_t* d = nullptr;
    unsigned dif_off[4] = {0, 0, 0, 0}, dit_off[4] = {0, 0, 0, 0};  // relative to d / to d + dit_base
    size_t dit_base = 0;
};
std::map<std::pair<int, int>, FusedTwiddles> g_fused_tw;  // (device, ka)

const FusedTwiddles* fused_twiddles(int ka, const GroupParams& ga, const GroupParams& gd) {
    return cached_table(g_fused_tw, ka, [&](std::vector<uint32_t>& h, FusedTwiddles& ft) {
        append_group_table(h, ga, true, ft.dif_off, 0);
        ft.dit_base = h.size();
        append_group_table(h, gd, false, ft.dit_off, ft.dit_base);
        return true;
    });
}

// The specialised kernel's table for height 2^n (lde_fused12_kernel): the two groups' tables at fixed offsets, the forward ones
// with the coset constant of their stage folded in — stage s of the size-2^(n+1) transform carries s^(2^(n-s)), so unlike
// FusedTwiddles this table depends on the height — the first forward stage times hinv = 1 / H as well, and every forward entry as
// its centred representative (|w| <= p / 2, an int32's bits): the kernel's forward rounds are signed. pw[e] = s^(2^e), e <= n.
struct Fused12Twiddles { uint32_t* d = nullptr; };
std::map<std::pair<int, int>, Fused12Twiddles> g_fused12_tw;  // (device, n)

const uint32_t* fused12_twiddles(int n, const GroupParams& ga, const GroupParams& gd, const uint32_t* pw, uint32_t hinv) {
    const Fused12Twiddles* ft = cached_table(g_fused12_tw, n, [&](std::vector<uint32_t>& h, Fused12Twiddles&) {
        unsigned dif_off[4] = {0, 0, 0, 0}, dit_off[4] = {0, 0, 0, 0};
        append_group_table(h, ga, true, dif_off, 0);
        if (h.size() > kF12D0) return false;
        h.resize(kF12D0, 0u);
        append_group_table(h, gd, false, dit_off, kF12D0);
        if (dif_off[0] != kF12A0 || dif_off[1] != kF12A1 || dif_off[2] != kF12A2 || dit_off[0] != 0 || kF12D0 + dit_off[1] != kF12D1 ||
            kF12D0 + dit_off[2] != kF12D2 || h.size() != kF12Words)
            return false;  // the kernel's constants and the planner disagree
        for (int r = 0; r < gd.n_rounds; ++r) {
            const size_t G = (size_t)1 << gd.rb[r];
            uint32_t* tab = h.data() + kF12D0 + dit_off[r];
            for (int q = 0; q < gd.logr[r]; ++q) {
                uint32_t cq = pw[n - (gd.s0 + gd.rb[r] - gd.c + q)];
                if (r == 0 && q == 0) cq = bb::mul(cq, hinv);  // D's first stage multiplies by 1 / H (lde_fused12_kernel)
                // centred (|w| <= p / 2), as the int32's bits: the forward rounds run bb::dit_signed
                for (size_t i = (((size_t)1 << q) - 1) * G; i < (((size_t)2 << q) - 1) * G; ++i) tab[i] = (uint32_t)bb::centred(bb::mul(tab[i], cq));
            }
        }
        return true;
    });
    return ft ? ft->d : nullptr;
}

}  // namespace

// The whole LDE of `cols` columns: natural-order evaluations on <g_n> (in) -> natural-order evaluations on the coset
// s <g_(n+1)> (out), through the fused middle kernel: strided DIF groups (stages 0 .. n-13, into `tmp`, which needs
// cols x 2^n words and is untouched when n <= 12), the fused kernel (the 12 contiguous DIF stages, scaling, duplication,
// 12 contiguous DIT stages: lde_fused12_kernel from 2^12 rows up, the generic lde_fused_kernel below), strided DIT groups in
// place on `out`. Same values as intt_dif + coset_lde_from_coeffs.
int lde_fused(const uint32_t* in, uint32_t* tmp, uint32_t* out, size_t in_stride, size_t tmp_stride, size_t out_stride, uint32_t cols, int n) {
    if (n == 0) {
        int rc = intt_dif(in, tmp, in_stride, tmp_stride, cols, n);
        return rc ? rc : coset_lde_from_coeffs(tmp, out, tmp_stride, out_stride, cols, n);
    }
    const Tables* tn = tables(n);
    const Tables* t1 = tables(n + 1);
    if (!tn || !t1) return (int)hipErrorOutOfMemory;
    const int ka = n < 12 ? n : 12;
    const char* force_generic = getenv("POWDR_LDE_FUSED_GENERIC");
    const bool spec12 = ka == 12 && !(force_generic && atoi(force_generic) != 0);
    // POWDR_NTT_STRIDED_GENERIC=1 (read per call): the strided groups stay on ntt_group_kernel at every height
    const char* strided_generic = getenv("POWDR_NTT_STRIDED_GENERIC");
    const bool strided_fixed = !(strided_generic && atoi(strided_generic) != 0);
    const uint32_t hinv = bb::inv(bb::to_monty((uint32_t)(((uint64_t)1 << n) % bb::P)));
    const uint32_t* src = in;
    size_t src_stride = in_stride;
    if (n > ka) {
        int logt = 12;
        auto groups = plan_groups(true, n, 0, logt, n - ka, true);
        launch_groups<true>(groups, logt, 0, in, tmp, in_stride, tmp_stride, cols, tn->tw_inv, nullptr, "ntt_group_kernel<dif>", nullptr, nullptr,
                            strided_fixed);
        src = tmp;
        src_stride = tmp_stride;
    }
    GroupParams ga = make_group(true, n, n - ka, ka, 0);
    GroupParams gd = make_group(false, n + 1, 1, ka, 1);
    gd.canonical_out = ka == n ? 1 : 0;
    // from 2^12 rows up the kernel specialised for the 12 + 12 geometry, which takes the coset scaling in its (and the strided DIT
    // groups') twiddles; POWDR_LDE_FUSED_GENERIC=1 keeps the generic kernel at every height
    uint32_t coset_pw[33];
    if (spec12) {
        coset_pw[0] = bb::to_monty(field::kCosetShift);
        for (int e = 1; e <= n; ++e) coset_pw[e] = bb::sqr(coset_pw[e - 1]);
        const uint32_t* tw12 = fused12_twiddles(n, ga, gd, coset_pw, hinv);
        if (!tw12) return (int)hipErrorOutOfMemory;
        const unsigned wgs = 1u << (n - 12);
        for_column_chunks(cols, [&](uint32_t c0, uint32_t cc) {
            ScopedKernelTimer t("lde_fused_kernel");
            const uint32_t* s_ = src + (size_t)c0 * src_stride;
            uint32_t* d_ = out + (size_t)c0 * out_stride;
            hipLaunchKernelGGL(lde_fused12_kernel, dim3(wgs, cc), dim3(kBlock), 0, stream(), s_, d_, src_stride, out_stride, tw12, bb::centred(hinv));
        });
    } else {
        const FusedTwiddles* ft = fused_twiddles(ka, ga, gd);
        if (!ft) return (int)hipErrorOutOfMemory;
        for (int r = 0; r < 4; ++r) { ga.twt_off[r] = ft->dif_off[r]; gd.twt_off[r] = ft->dit_off[r]; }
        const unsigned wgs = (unsigned)div_up((size_t)ga.n_tiles, (size_t)1 << (12 - ka));
        for_column_chunks(cols, [&](uint32_t c0, uint32_t cc) {
            ScopedKernelTimer t("lde_fused_kernel");
            hipLaunchKernelGGL(lde_fused_kernel, dim3(wgs, cc), dim3(kBlock), 0, stream(), src + (size_t)c0 * src_stride,
                               out + (size_t)c0 * out_stride, src_stride, out_stride, ga, gd, ft->d, ft->d + ft->dit_base, tn->shift_br);
        });
    }
    if (n > ka) {
        int logt = 12;
        auto groups = plan_groups(false, n + 1, ka + 1, logt, n + 1, true);
        if (!groups.empty()) groups.back().canonical_out = 1;
        launch_groups<false>(groups, logt, 0, out, out, out_stride, out_stride, cols, t1->tw_fwd, nullptr, "ntt_group_kernel<dit>", nullptr,
                             spec12 ? coset_pw : nullptr, strided_fixed);
    }
    return (int)hipGetLastError();
}

// Unscaled inverse NTT: natural-order evaluations on <g_n> -> bit-reversed coefficient order,
// out[q] = 2^n * coefficient[bitrev(q)].
int intt_dif(const uint32_t* in, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n) {
    const Tables* t = tables(n);
    if (!t) return (int)hipErrorOutOfMemory;
    run_groups<true>(in, out, in_stride, out_stride, cols, n, 0, t->tw_inv, nullptr, "ntt_group_kernel<dif>");
    return (int)hipGetLastError();
}

// coeffs: bit-reversed order, scaled by 2^n (as intt_dif leaves them). out: 2^(n+1) natural-order
// evaluations on the coset s*<g_{n+1}>.
int coset_lde_from_coeffs(const uint32_t* coeffs, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n) {
    const Tables* tn = tables(n);
    const Tables* t1 = tables(n + 1);
    if (!tn || !t1) return (int)hipErrorOutOfMemory;
    if (n == 0) {
        ScopedKernelTimer t("expand_small_kernel");
        hipLaunchKernelGGL(expand_small_kernel, dim3(1, cols), dim3(64), 0, stream(), coeffs, out, in_stride, out_stride,
                           (size_t)1, tn->shift_br);
        return (int)hipGetLastError();
    }
    // stage 0 of the size-2^(n+1) DIT is the duplication done by the EXPAND load of the first group
    run_groups<false>(coeffs, out, in_stride, out_stride, cols, n + 1, 1, t1->tw_fwd, tn->shift_br, "ntt_group_kernel<dit>");
    return (int)hipGetLastError();
}

// ---- sub-coset evaluation (the streamed prover, prover.hip "streamed proofs") ---------------------------------------------
// The LDE domain s <g_(n+1)> (2^(n+1) points) is the union of 2^b sub-cosets c <g_m>, c = s g_(n+1)^r, m = 2^(n+1-b), r < 2^b: rows
// j = r + 2^b i of the LDE. On one of them x^m is the constant c^m, so a polynomial of degree < 2^n is its remainder modulo
// x^m - c^m there: b_i = sum_t a_(i + t m) c^(t m), 2^(b-1) coefficients per position — contiguous in the bit-reversed order of the
// coefficient arrays, their factors the same for every position (kernel arguments) — and the remainder is evaluated on c <g_m> by a
// size-m COSET transform: the DIT network with the twiddles of stage s multiplied by c^(2^(log2 m - 1 - s)) (P(x) = E(x^2) + x O(x^2)
// level by level), i.e. no scaling pass and no per-element scale table. Work per column and sub-coset: 2^n multiply-adds +
// (m / 2) log2 m butterflies; all 2^b sub-cosets together read the coefficients 2^(b-1) times for one forward transform's butterflies.
namespace {
// the sub-coset's constants: c = s g_(n+1)^r; C[s] = c^(2^(nm-1-s)); fold factors (c^m)^bitrev(t) / H
bool subcoset_spec(int n, int b, uint32_t r, uint32_t* d_scratch, CosetSpec& cs) {
    const int nm = n + 1 - b;
    if (b < 1 || b > 5 || nm < 1 || (r >> b)) return false;
    cs = CosetSpec{};
    cs.fold_log = b - 1;
    cs.d_scratch = d_scratch;
    uint32_t pw[32];
    pw[0] = bb::mul(bb::to_monty(field::kCosetShift), bb::pow_u32(field::root_of_unity(n + 1), r));
    for (int e = 1; e <= nm; ++e) pw[e] = bb::sqr(pw[e - 1]);
    for (int s = 0; s < nm; ++s) cs.C[s] = pw[nm - 1 - s];
    const uint32_t hinv = bb::inv(bb::to_monty((uint32_t)(((uint64_t)1 << n) % bb::P)));  // the coefficient arrays are H-scaled
    const int f = b - 1;
    for (uint32_t tp = 0; tp < (1u << f); ++tp) {
        const uint32_t t = f ? (__builtin_bitreverse32(tp) >> (32 - f)) : 0u;
        cs.foldk[tp] = bb::mul(bb::pow_u32(pw[nm], t), hinv);
    }
    return true;
}

// After the first `k1` DIT stages block t of 2^k1 contiguous elements holds P_u(y), u = bitrev(t), on the points y = x^(2^k2) of its
// own coset, where P(x) = sum_u x^u P_u(x^(2^k2)), k2 = nm - k1. Output i of the whole transform is then a 2^k2-term sum:
//   out[i] = sum_u x_i^u part[bitrev_k2(u) * 2^k1 + (i mod 2^k1)],  x_i = c w_m^i
// — what the remaining (strided) stages compute for EVERY i; the query phase needs ~a hundred of them. One thread per (row, column).
// The partial values are the forward network's [0, 2p) representatives.
__global__ __launch_bounds__(256) void subcoset_rows_kernel(const uint32_t* __restrict__ part, size_t stride, uint32_t cols, int k1, int k2, uint32_t c0,
                                                            uint32_t wm, const uint32_t* __restrict__ idx, const uint32_t* __restrict__ slot,
                                                            uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= cols) return;
    const uint32_t i = idx[blockIdx.y];
    const uint32_t x = bb::mul(c0, bb::pow_u32(wm, i));
    const uint32_t* col = part + (size_t)c * stride + (i & ((1u << k1) - 1u));
    uint32_t acc = 0u, xp = bb::R_MOD_P;
    for (uint32_t u = 0; u < (1u << k2); ++u) {
        const uint32_t t = k2 ? (__brev(u) >> (32 - k2)) : 0u;
        acc = bb::add(acc, bb::mul(bb::reduce_2p(col[(size_t)t << k1]), xp));
        xp = bb::mul(xp, x);
    }
    out[(size_t)(slot ? slot[blockIdx.y] : blockIdx.y) * cols + c] = acc;
}
// xpow[q * n_tiles + t] = x_q^(bitrev_k2(t)), x_q = c0 wm^(idx[q]): the factor tile t's element contributes to output idx[q] with
__global__ __launch_bounds__(256) void select_xpow_kernel(const uint32_t* __restrict__ idx, uint32_t n_idx, int k2, uint32_t c0, uint32_t wm,
                                                         uint32_t* __restrict__ xpow, uint32_t* __restrict__ pos, uint32_t pos_mask) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const size_t n_tiles = (size_t)1 << k2;
    if (gid >= (size_t)n_idx * n_tiles) return;
    const uint32_t q = (uint32_t)(gid >> k2), t = (uint32_t)(gid & (n_tiles - 1));
    const uint32_t i = idx[q];
    const uint32_t x = bb::mul(c0, bb::pow_u32(wm, i));
    const uint32_t u = k2 ? (__brev(t) >> (32 - k2)) : 0u;
    xpow[gid] = bb::pow_u32(x, u);
    if (t == 0) pos[q] = i & pos_mask;
}

// rows_out[slot(q) * cols + c] = acc[c * n + q] mod p, as a Montgomery word in [0, p)
__global__ __launch_bounds__(256) void select_finish_kernel(const unsigned long long* __restrict__ acc, uint32_t n, uint32_t cols,
                                                           const uint32_t* __restrict__ slot, uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= cols) return;
    const uint32_t q = blockIdx.y;
    out[(size_t)(slot ? slot[q] : q) * cols + c] = (uint32_t)(acc[(size_t)c * n + q] % bb::P);
}
// rows_out[slot(q) * cols + c] = sum_t part[(c * n_tiles + t) * n + q] mod p: lane = output q (a tile's n terms are consecutive words),
// the tiles of the column one after the other. 2^k2 <= 2^14 terms below p: the sum fits 64 bits with room to spare.
__global__ __launch_bounds__(128) void select_reduce_kernel(const uint32_t* __restrict__ part, uint32_t n, uint32_t cols, size_t n_tiles,
                                                           const uint32_t* __restrict__ slot, uint32_t* __restrict__ out) {
    const uint32_t q = blockIdx.x * 128u + threadIdx.x, c = blockIdx.y;
    if (q >= n) return;
    const uint32_t* col = part + (size_t)c * n_tiles * n + q;
    unsigned long long acc = 0;
#pragma unroll 8
    for (size_t t = 0; t < n_tiles; ++t) acc += col[t * n];
    out[(size_t)(slot ? slot[q] : q) * cols + c] = (uint32_t)(acc % bb::P);
}
}  // namespace

// The rows d_local_idx[q] (q < n_idx) of sub-coset r's LDE WITHOUT storing the partial transform: the first stage group with SELECT
// (the tile stays in LDS, every selected output gets this tile's term through a 64-bit atomic sum) — the query phase of a streamed
// proof reads the coefficients once and writes a few megabytes. Tall transforms only (one 2^12-tile per workgroup and at least one
// strided stage left); returns 1 when the shape does not qualify and nothing was done (the caller then takes
// subcoset_lde_first_group + subcoset_rows). d_work: 2^13 + n_idx * (2^k2 + 1) words (each of the two terms rounded up to even) +
// cols * n_idx 64-bit sums; the stored-terms form takes cols * 2^k2 * n_idx words more. *form_out: prover_internal.hpp.
int subcoset_query_rows(const uint32_t* coeffs, size_t in_stride, uint32_t cols, int n, int b, uint32_t r, const uint32_t* d_local_idx,
                        uint32_t n_idx, const uint32_t* d_slot, uint32_t* rows_out, uint32_t* d_work, size_t work_words, int* form_out) {
    const int nm = n + 1 - b;
    if (form_out) *form_out = 0;
    if (!n_idx || !cols) return 0;
    if (cols > 65535u) return 1;  // (one launch: blockIdx.y is the column)
    // POWDR_QUERY_SELECT: 0 = never (the stored partial transform + subcoset_rows), 2 = round 5's 64-bit atomic sums, default (1) =
    // every workgroup STORES its n_idx terms and select_reduce_kernel adds a column's tiles: the same words, no atomics — tiles x cols x
    // n_idx of them per pass (4.3e8 at configs[2]), all tiles of a column on the same n_idx addresses — and a kernel that profiles
    // under rocprofv3 --pmc (the atomic form's FETCH_SIZE pass did not return: DESIGN §3.8 round 6, tools/repro_select_atomics.py)
    const int sel_mode = getenv("POWDR_QUERY_SELECT") ? atoi(getenv("POWDR_QUERY_SELECT")) : 1;
    if (sel_mode == 0) return 1;
    CosetSpec cs;
    if (!subcoset_spec(n, b, r, d_work, cs)) return (int)hipErrorInvalidValue;
    int logt = 12;
    auto groups = plan_groups(false, nm, 0, logt);
    if (groups.size() < 2 || logt != 12 || groups[0].B != 12 || groups[0].c != 0 || groups[0].lowbits != 0 || cs.fold_log > 1) return 1;
    const int k1 = groups[0].k, k2 = nm - k1;
    const size_t n_tiles = (size_t)1 << k2;
    uint32_t* d_pos = d_work + (1u << 13);
    uint32_t* d_xpow = d_pos + ((n_idx + 1u) & ~1u);
    unsigned long long* d_acc = reinterpret_cast<unsigned long long*>(d_xpow + (((size_t)n_idx * n_tiles + 1) & ~(size_t)1));
    uint32_t* d_part = reinterpret_cast<uint32_t*>(d_acc + (size_t)cols * n_idx);
    bool partial = sel_mode != 2;
    size_t need = (size_t)(d_part - d_work) + (partial ? (size_t)cols * n_tiles * n_idx : 0);
    if (partial && need > work_words) { partial = false; need = (size_t)(d_part - d_work); }  // (no room for the terms: the atomic sums)
    if (need > work_words || ((uintptr_t)d_work & 7)) return 1;
    const Tables* tm = tables(nm);
    if (!tm) return (int)hipErrorOutOfMemory;
    const uint32_t c0 = bb::mul(bb::to_monty(field::kCosetShift), bb::pow_u32(field::root_of_unity(n + 1), r));
    {
        ScopedKernelTimer t("subcoset_rows_kernel");
        hipLaunchKernelGGL(select_xpow_kernel, dim3((unsigned)div_up((size_t)n_idx * n_tiles, 256)), dim3(256), 0, stream(), d_local_idx, n_idx, k2, c0,
                           field::root_of_unity(nm), d_xpow, d_pos, (1u << k1) - 1u);
    }
    if (!partial) PW_HIP_TRY(hipMemsetAsync(d_acc, 0, (size_t)cols * n_idx * sizeof(unsigned long long), stream()));
    if (form_out) *form_out = partial ? 1 : 2;
    cs.n_sel = (int)n_idx; cs.sel_pos = d_pos; cs.sel_xpow = d_xpow; cs.sel_acc = d_acc; cs.sel_part = partial ? d_part : nullptr;
    int done = 0;
    // (`out` of the group is never written in SELECT mode: the coefficient array stands in for it)
    run_groups<false>(coeffs, const_cast<uint32_t*>(coeffs), in_stride, in_stride, cols, nm, 0, tm->tw_fwd, nullptr, "ntt_group_kernel<dit>", &cs, 1, &done);
    {
        ScopedKernelTimer t("subcoset_rows_kernel");
        if (partial) hipLaunchKernelGGL(select_reduce_kernel, dim3(div_up(n_idx, 128), cols), dim3(128), 0, stream(), d_part, n_idx, cols, n_tiles, d_slot, rows_out);
        else hipLaunchKernelGGL(select_finish_kernel, dim3(div_up(cols, 256), n_idx), dim3(256), 0, stream(), d_acc, n_idx, cols, d_slot, rows_out);
    }
    return (int)hipGetLastError();
}

int subcoset_lde(const uint32_t* coeffs, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n, int b, uint32_t r,
                 uint32_t* d_scratch) {
    const int nm = n + 1 - b;  // log2 of the sub-coset's size
    CosetSpec cs;
    if (!subcoset_spec(n, b, r, d_scratch, cs)) return (int)hipErrorInvalidValue;
    const Tables* tm = tables(nm);
    if (!tm) return (int)hipErrorOutOfMemory;
    run_groups<false>(coeffs, out, in_stride, out_stride, cols, nm, 0, tm->tw_fwd, nullptr, "ntt_group_kernel<dit>", &cs);
    return (int)hipGetLastError();
}

// Coefficient arrays as intt_dif leaves them (bit-reversed, H-scaled) back to the values on <g_n>, natural order, canonical words: the
// forward network of subcoset_lde with the trivial coset (every stage constant 1) and the single "fold" factor 1/H. In place or not.
int values_from_coefficients(const uint32_t* coeffs, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n, uint32_t* d_scratch) {
    if (n < 1 || n > 26) return (int)hipErrorInvalidValue;
    CosetSpec cs{};
    cs.fold_log = 0;
    cs.d_scratch = d_scratch;
    for (int s = 0; s < 32; ++s) cs.C[s] = bb::R_MOD_P;
    cs.foldk[0] = bb::inv(bb::to_monty((uint32_t)(((uint64_t)1 << n) % bb::P)));
    const Tables* tn = tables(n);
    if (!tn) return (int)hipErrorOutOfMemory;
    run_groups<false>(coeffs, out, in_stride, out_stride, cols, n, 0, tn->tw_fwd, nullptr, "ntt_group_kernel<dit>", &cs);
    return (int)hipGetLastError();
}

// Only the first stage group of subcoset_lde (the contiguous stages, with the FOLD loads): `out` holds the PARTIAL transform,
// *stages_done stages of log2 m. subcoset_rows finishes it for chosen rows.
int subcoset_lde_first_group(const uint32_t* coeffs, uint32_t* out, size_t in_stride, size_t out_stride, uint32_t cols, int n, int b, uint32_t r,
                             uint32_t* d_scratch, int* stages_done) {
    const int nm = n + 1 - b;
    CosetSpec cs;
    if (!subcoset_spec(n, b, r, d_scratch, cs) || !stages_done) return (int)hipErrorInvalidValue;
    const Tables* tm = tables(nm);
    if (!tm) return (int)hipErrorOutOfMemory;
    run_groups<false>(coeffs, out, in_stride, out_stride, cols, nm, 0, tm->tw_fwd, nullptr, "ntt_group_kernel<dit>", &cs, 1, stages_done);
    return (int)hipGetLastError();
}

// out[slot(q) * cols + c] = row d_local_idx[q] of the sub-coset's LDE (canonical Montgomery words), from the partial transform;
// slot(q) = d_slot[q], or q when d_slot is null
int subcoset_rows(const uint32_t* part, size_t stride, uint32_t cols, int n, int b, uint32_t r, int stages_done, const uint32_t* d_local_idx,
                  uint32_t n_idx, const uint32_t* d_slot, uint32_t* out) {
    const int nm = n + 1 - b;
    if (!n_idx || !cols) return 0;
    if (stages_done < 0 || stages_done > nm) return (int)hipErrorInvalidValue;
    const uint32_t c0 = bb::mul(bb::to_monty(field::kCosetShift), bb::pow_u32(field::root_of_unity(n + 1), r));
    ScopedKernelTimer t("subcoset_rows_kernel");
    hipLaunchKernelGGL(subcoset_rows_kernel, dim3(div_up(cols, 256), n_idx), dim3(256), 0, stream(), part, stride, cols, stages_done, nm - stages_done, c0,
                       field::root_of_unity(nm), d_local_idx, d_slot, out);
    return (int)hipGetLastError();
}

}  // namespace pw
