// Device-side generation of the traces of the system AIRs that close a segment's buses (include/powdr_prover.h
// pw_program_frequencies / pw_memory_boundary_trace; the AIRs themselves: powdr_amd/system_airs.py).
//   program     program_freq_kernel   every active (air, interaction on the PC-lookup bus, row) is matched word for word against the
//                                     row (pc - pc_base) / pc_step of the program table and adds its centred multiplicity to that
//                                     row's sum — merged per wave, then per workgroup in LDS (the first kFreqLdsBins rows) — or is
//                                     counted as foreign; program_freq_finish_kernel reduces the sums mod p
//   boundary    boundary_walk_kernel  pass 1: (as, ptr) of every active triple of the memory bus into an open-addressing table keyed
//                                     by ADDRESS, atomicMin of the timestamp over the receives, atomicMax over the sends; pass 2:
//                                     atomicMin of the packed witness over the triples that carry those extremes;
//                                     boundary_compact_kernel + a radix sort of the keys; boundary_rows_kernel: one lane per row
//                                     re-evaluates the data words at the two witnesses and writes the 18 columns
//   poseidon2   compress_tally_kernel every active triple of the compression bus into an open-addressing table keyed by the fingerprint
//                                     of its 16 INPUT words (the digest words are not read): 64-bit sum of the centred multiplicities,
//                                     atomicMin of the packed witness; compress_compact_kernel + a radix sort of (witness, sum);
//                                     compress_rows_kernel: one lane per row re-evaluates the inputs at the witness and runs a
//                                     permutation that stores every committed intermediate
// One lane per row, interactions evaluated by eval_span exactly as the prover and the bus check evaluate them. Both tables are the
// bus check's (bus_shared.hpp: the claim loop, the load rule, the sizing and the growth), each with its own payload columns.
#include "scratch.hpp"
#include "bus_witness_args.hpp"
#include "prover_internal.hpp"

#include <rocprim/rocprim.hpp>

namespace pw {

namespace {

using namespace bus;

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kFreqLdsBins = 4096;    // 32 KB of 64-bit sums next to the interpreter's 16 KB stack
constexpr int kFreqMergeRounds = 4;        // distinct table rows a wave merges before its lanes fall back to one atomic each
constexpr uint32_t kProgramArgs = 9;       // pc, opcode, a .. g
constexpr uint32_t kMemoryArgs = 7;        // as, ptr, four data words, timestamp
constexpr uint32_t kBoundaryWidth = 18;
constexpr uint32_t kLimbBits = 17;
// what a walk found wrong with the multiplicities (boundary_walk_kernel)
constexpr uint32_t kFlagMagnitude = 1u;

// ---- the program AIR's multiplicities ----------------------------------------------------------------------------------------------
// sums[row] += the centred multiplicities of the tuples that equal program row `row` (two's complement in 64 bits: exact below 2^32
// contributions per row); foreign[0] += tuples that equal no row, foreign[1] = min of their packed witnesses, foreign[2 .. 4] statistics. A lane walks
// rows_per_lane rows (row = first + k * kBlock: coalesced). The loops are wave-uniform (a lane past the end carries no tuple), so that
// the lanes of a wave can merge: the rows of an instruction AIR repeat a block's few instructions, a wave of 64 consecutive rows holds
// a handful of distinct table rows, and each of them costs ONE atomic per wave — into LDS for the first kFreqLdsBins table rows (a loop
// body lies there when pc_base is its first pc), one global atomic per (workgroup, row) at the end.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void program_freq_kernel(const uint32_t* __restrict__ m, size_t H, uint32_t rows_per_lane, LogupProgram lp,
                                                               const uint32_t* __restrict__ order, uint32_t begin, uint32_t end, uint32_t air,
                                                               uint32_t pc_base, uint32_t pc_step, const uint32_t* __restrict__ program, uint32_t table_rows,
                                                               u64* __restrict__ sums, u64* __restrict__ foreign) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    __shared__ u64 bins[kFreqLdsBins];
    uint32_t* stk = stack_lds + threadIdx.x;
    for (uint32_t b = threadIdx.x; b < kFreqLdsBins; b += kBlock) bins[b] = 0;
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * kBlock * rows_per_lane + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    u64 n_foreign = 0, w_foreign = kEmpty, n_active = 0, n_lds = 0, n_global = 0;
    for (uint32_t k = 0; k < rows_per_lane; ++k) {
        const size_t r = first + (size_t)k * kBlock;
        for (uint32_t i = begin; i < end; ++i) {
            const uint32_t idx = order[i];
            const LogupInteraction it = lp.d_inter[idx];
            uint32_t bin = kNone;
            long long cm = 0;
            const uint32_t mu = r < H ? eval_span<FAST>(lp, it.first_span, m, H, r, stk) : 0u;
            if (mu != 0u) {
                ++n_active;
                cm = (long long)bb::centred(bb::from_monty(mu));
                bool ok = it.n_args == kProgramArgs;
                if (ok) {
                    const uint32_t pc = bb::from_monty(eval_span<FAST>(lp, it.first_span + 1, m, H, r, stk));
                    ok = pc >= pc_base && (pc - pc_base) % pc_step == 0u && (pc - pc_base) / pc_step < table_rows;
                    if (ok) {
                        const uint32_t row = (pc - pc_base) / pc_step;
                        ok = bb::from_monty(program[row]) == pc;
                        for (uint32_t j = 1; ok && j < kProgramArgs; ++j)
                            ok = bb::from_monty(eval_span<FAST>(lp, it.first_span + 1 + j, m, H, r, stk)) == bb::from_monty(program[(size_t)j * table_rows + row]);
                        if (ok) bin = row;
                    }
                }
                if (!ok) {
                    ++n_foreign;
                    const u64 w = pack_witness(air, idx, r);
                    w_foreign = w < w_foreign ? w : w_foreign;
                }
            }
            u64 todo = __builtin_amdgcn_ballot_w64(bin != kNone);
            for (int round = 0; round < kFreqMergeRounds && todo; ++round) {
                const int leader = __builtin_ctzll(todo);
                const uint32_t key = (uint32_t)__shfl((int)bin, leader, 64);
                const bool mine = bin == key;
                const u64 s = wave_sum(mine ? (u64)cm : 0ull);
                if (lane == (unsigned)leader) {
                    if (key < kFreqLdsBins) { atomicAdd(&bins[key], s); ++n_lds; }
                    else { atomicAdd(sums + key, s); ++n_global; }
                }
                todo &= ~__builtin_amdgcn_ballot_w64(mine);
            }
            if ((todo >> lane) & 1ull) {  // (a wave with many distinct rows: straight-line code)
                if (bin < kFreqLdsBins) { atomicAdd(&bins[bin], (u64)cm); ++n_lds; }
                else { atomicAdd(sums + bin, (u64)cm); ++n_global; }
            }
        }
    }
    n_foreign = wave_sum(n_foreign);
    w_foreign = wave_min(w_foreign);
    if (lane == 0 && n_foreign) {
        atomicAdd(foreign, n_foreign);
        atomicMin(foreign + 1, w_foreign);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kFreqLdsBins && b < table_rows; b += kBlock)
        if (bins[b]) { atomicAdd(sums + b, bins[b]); ++n_global; }
    // what the call did, for pw_system_traces_last_stats: additions asked for, LDS and global atomics issued (three atomics per wave)
    n_active = wave_sum(n_active);
    n_lds = wave_sum(n_lds);
    n_global = wave_sum(n_global);
    if (lane == 0) {
        if (n_active) atomicAdd(foreign + 2, n_active);
        if (n_lds) atomicAdd(foreign + 3, n_lds);
        if (n_global) atomicAdd(foreign + 4, n_global);
    }
}

__global__ __launch_bounds__(kBlock) void program_freq_finish_kernel(const u64* __restrict__ sums, uint32_t table_rows, uint32_t* __restrict__ freq) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= table_rows) return;
    freq[r] = bb::to_monty(sum_residue(sums[r]));
}

// ---- the memory boundary AIR's trace -----------------------------------------------------------------------------------------------
// one slot per touched location: the key (as << 32 | ptr: one key word, v.k1 unused), the smallest timestamp a receive carried (what
// the location held before its first access: kEmpty = no receive), the largest a send carried + 1 (what it holds after its last: 0 =
// no send), and the smallest packed witness among the triples that carry each extreme
struct AddrTable { TableView v; u64 *tmin, *wmin, *wmax, *tmax; };

__device__ __forceinline__ u64 address_key(uint32_t as, uint32_t ptr) { return ((u64)as << 32) | (u64)ptr; }

// PASS 1: claim the slot of every active triple's address (claim_slot, bus_shared.hpp) and fold the timestamp in. PASS 2: the same
// walk; a triple whose timestamp is its slot's extreme offers its witness (every key it asks for was inserted). A multiplicity that
// is not +1 or -1 sets kFlagMagnitude and is left out.
template <bool FAST, int PASS>
__global__ __launch_bounds__(kBlock) void boundary_walk_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                                uint32_t begin, uint32_t end, uint32_t air, AddrTable t, uint32_t* __restrict__ overflow,
                                                                uint32_t* __restrict__ flags) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= H || __atomic_load_n(overflow, __ATOMIC_RELAXED)) return;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t idx = order[i];
        const LogupInteraction it = lp.d_inter[idx];
        const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
        if (mu == 0u) continue;
        const int32_t cm = bb::centred(bb::from_monty(mu));
        if (cm != 1 && cm != -1) {
            if (PASS == 1) atomicOr(flags, kFlagMagnitude);
            continue;
        }
        const uint32_t as = bb::from_monty(eval_span<FAST>(lp, it.first_span + 1, m, H, r, stk));
        const uint32_t ptr = bb::from_monty(eval_span<FAST>(lp, it.first_span + 2, m, H, r, stk));
        const u64 ts = bb::from_monty(eval_span<FAST>(lp, it.first_span + it.n_args, m, H, r, stk));
        const u64 key = address_key(as, ptr);
        if (PASS == 2) {
            const u64 s = find_slot(t.v, key);
            if (s == kEmpty) continue;
            const u64 w = pack_witness(air, idx, r);
            if (cm < 0) {
                if (t.tmin[s] == ts) atomicMin(t.wmin + s, w);
            } else if (t.tmax[s] == ts + 1) {
                atomicMin(t.wmax + s, w);
            }
            continue;
        }
        const u64 s = claim_slot<1>(t.v, key, 0, overflow);
        if (s == kEmpty) return;
        // (a register is touched by every call: most triples lose against what the slot already holds and cost a load)
        if (cm < 0) {
            if (__atomic_load_n(t.tmin + s, __ATOMIC_RELAXED) > ts) atomicMin(t.tmin + s, ts);
        } else if (__atomic_load_n(t.tmax + s, __ATOMIC_RELAXED) < ts + 1) {
            atomicMax(t.tmax + s, ts + 1);
        }
    }
}

// counts[0] = occupied slots, counts[1] = those with only receives or only sends; with `keys`: the occupied slots' keys, in arrival
// order (sorted afterwards), counts[2] = written
__global__ __launch_bounds__(kBlock) void boundary_compact_kernel(AddrTable t, u64* __restrict__ keys, u64 cap, u64* __restrict__ counts) {
    const u64 s = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (s > t.v.mask || t.v.k0[s] == kEmpty) return;
    if (!keys) {
        atomicAdd(counts, 1ull);
        if (t.tmin[s] == kEmpty || t.tmax[s] == 0ull) atomicAdd(counts + 1, 1ull);
        return;
    }
    const u64 at = atomicAdd(counts + 2, 1ull);
    if (at < cap) keys[at] = t.v.k0[s];
}

__device__ __forceinline__ uint32_t witness_arg(const AirDev* __restrict__ airs, u64 w, uint32_t j, uint32_t* stk) {
    const Witness at = unpack_witness(w);
    const AirDev a = airs[at.air];
    return eval_span_of(a, a.lp.d_inter[at.inter].first_span + 1 + j, at.row, stk);
}

// Row r of the boundary trace (column-major, H_out rows, Montgomery) from the r-th smallest address: [is_valid, as, ptr, p_lo, p_hi,
// init0..3, init_ts, fin0..3, fin_ts, same_as, d_lo, d_hi]; the gap to the next address and same_as from the sorted neighbour, the
// data words re-evaluated at the two witness rows (lanes of a wave may run different programs: correct, and the rows are few next to
// the walks). Rows from n on are zero.
__global__ __launch_bounds__(kBlock) void boundary_rows_kernel(const u64* __restrict__ sorted, u64 n, AddrTable t, const AirDev* __restrict__ airs,
                                                                size_t H_out, uint32_t* __restrict__ out) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= H_out) return;
    uint32_t v[kBoundaryWidth];
#pragma unroll
    for (uint32_t c = 0; c < kBoundaryWidth; ++c) v[c] = 0u;
    if (r < n) {
        const u64 key = sorted[r];
        const uint32_t as = (uint32_t)(key >> 32), ptr = (uint32_t)key;
        const u64 s = find_slot(t.v, key);
        v[0] = bb::to_monty(1u);
        v[1] = bb::to_monty(as);
        v[2] = bb::to_monty(ptr);
        v[3] = bb::to_monty(ptr & ((1u << kLimbBits) - 1u));
        v[4] = bb::to_monty(ptr >> kLimbBits);
        if (s != kEmpty) {
            const u64 wmin = t.wmin[s], wmax = t.wmax[s];
            for (uint32_t j = 0; j < 4 && wmin != kEmpty && wmax != kEmpty; ++j) {  // (both exist: the host has refused status 4)
                v[5 + j] = witness_arg(airs, wmin, 2 + j, stk);
                v[10 + j] = witness_arg(airs, wmax, 2 + j, stk);
            }
            v[9] = bb::to_monty((uint32_t)t.tmin[s]);
            v[14] = bb::to_monty((uint32_t)(t.tmax[s] - 1));
        }
        if (r + 1 < n) {
            const u64 next = sorted[r + 1];
            if ((uint32_t)(next >> 32) == as) {
                const uint32_t d = (uint32_t)next - ptr - 1u;
                v[15] = bb::to_monty(1u);
                v[16] = bb::to_monty(d & ((1u << kLimbBits) - 1u));
                v[17] = bb::to_monty(d >> kLimbBits);
            }
        }
    }
#pragma unroll
    for (uint32_t c = 0; c < kBoundaryWidth; ++c) out[(size_t)c * H_out + r] = v[c];
}

// ---- the Poseidon2 compression chip's trace -----------------------------------------------------------------------------------------
constexpr uint32_t kCompressArgs = 24, kCompressIn = 16;  // left[8], right[8], out[8]: the key is the 16 input words
constexpr uint32_t kP2Width = 307;                         // mult | in[16] | 8 x (cube[16], sbox[16]) | 13 x (pcube, psbox) | out[8]
constexpr uint32_t kP2In = 1, kP2Full = 17, kP2Partial = kP2Full + 8 * 32, kP2Out = kP2Partial + 2 * 13;
constexpr size_t kP2SlotBytes = 32;                        // key 2 x 8, sum 8, witness 8
static_assert(kP2Out + 8 == kP2Width, "the layout of powdr_amd/system_airs.py poseidon2_air");

// the definition of the installed permutation (Montgomery words) and the challenges of the key's fingerprint: kernel arguments, so
// the round constants arrive through scalar loads indexed by the wave-uniform round counter
struct P2Def { uint32_t ext_rc[8][16]; uint32_t int_rc[13]; uint32_t diag[16]; };
struct P2Key { bb::Ext al; bb::Ext blpow[kCompressIn + 1]; };
struct P2Table { TableView v; u64 *sum, *wit; };

// bus_tally_kernel with the key cut down to the inputs: every active (interaction, row) of the compression bus in one AIR adds its
// centred multiplicity to the slot of the fingerprint al + sum_j bl^(j+1) in_j (j < 16; 124 bits, the two key words of claim_slot,
// bus_shared.hpp) and offers its packed witness. Keys never change once set, sums are integer additions and the witness is a
// minimum: what a slot ends with does not depend on the order of arrival.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void compress_tally_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                                 uint32_t begin, uint32_t end, uint32_t air, P2Key key, P2Table t,
                                                                 uint32_t* __restrict__ overflow) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= H || __atomic_load_n(overflow, __ATOMIC_RELAXED)) return;
    const pwj::DenominatorSeeds sd = pwj::denominator_seeds(key.al);
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t idx = order[i];
        const LogupInteraction it = lp.d_inter[idx];
        const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
        if (mu == 0u) continue;
        pwj::DenominatorAcc acc(sd, 0u);
        for (uint32_t j = 0; j < kCompressIn; ++j) acc.add(eval_span<FAST>(lp, it.first_span + 1 + j, m, H, r, stk), key.blpow[j + 1]);
        const bb::Ext d = acc.result();
        const u64 a = (u64)d.c[0] | ((u64)d.c[1] << 32), b = (u64)d.c[2] | ((u64)d.c[3] << 32);
        const u64 witness = pack_witness(air, idx, r);
        const long long cm = (long long)bb::centred(bb::from_monty(mu));
        const u64 s = claim_slot<2>(t.v, a, b, overflow);
        if (s == kEmpty) return;
        atomicAdd(t.sum + s, (u64)cm);
        atomicMin(t.wit + s, witness);
    }
}

// counts[0] = occupied slots; with `wit`: their (witness, sum) pairs in arrival order (sorted afterwards), counts[2] = written. One
// atomic per wave: the occupied lanes of a wave are counted by a ballot and take consecutive places behind the leader's.
__global__ __launch_bounds__(kBlock) void compress_compact_kernel(P2Table t, u64* __restrict__ wit, u64* __restrict__ sum, u64 cap, u64* __restrict__ counts) {
    const u64 s = (u64)blockIdx.x * kBlock + threadIdx.x;
    const bool occupied = s <= t.v.mask && t.v.k0[s] != kEmpty;
    const u64 lanes = __builtin_amdgcn_ballot_w64(occupied);
    if (!lanes) return;
    const unsigned lane = threadIdx.x & 63u;
    const int leader = __builtin_ctzll(lanes);
    u64 base = 0;
    if ((int)lane == leader) base = atomicAdd(counts + (wit ? 2 : 0), (u64)__builtin_popcountll(lanes));
    if (!wit || !occupied) return;
    base = ((u64)(uint32_t)__shfl((int)(base >> 32), leader, 64) << 32) | (u64)(uint32_t)__shfl((int)base, leader, 64);
    const u64 at = base + (u64)__builtin_popcountll(lanes & ((1ull << lane) - 1ull));
    if (at < cap) {
        wit[at] = t.wit[s];
        sum[at] = t.sum[s];
    }
}

// the external layer on canonical Montgomery words: M4 on each block of four through its shared partial sums (poseidon2.hpp
// external_layer), then every word gets its column's sum over the four blocks
__device__ __forceinline__ void p2_external_plain(uint32_t* s) {
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t x0 = s[4 * b], x1 = s[4 * b + 1], x2 = s[4 * b + 2], x3 = s[4 * b + 3];
        const uint32_t t01 = bb::add(x0, x1), t23 = bb::add(x2, x3), t = bb::add(t01, t23);
        const uint32_t ta = bb::add(t, x1), tb = bb::add(t, x3);
        s[4 * b] = bb::add(ta, t01);
        s[4 * b + 1] = bb::add(ta, bb::double_(x2));
        s[4 * b + 2] = bb::add(tb, t23);
        s[4 * b + 3] = bb::add(tb, bb::double_(x0));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t col = bb::add(bb::add(s[i], s[4 + i]), bb::add(s[8 + i], s[12 + i]));
#pragma unroll
        for (int b = 0; b < 4; ++b) s[4 * b + i] = bb::add(s[4 * b + i], col);
    }
}

// x -> x^7 with x^3 and x^7 stored where the AIR commits them (x = the S-box input, its round constant added)
__device__ __forceinline__ uint32_t p2_sbox_record(uint32_t x, uint32_t* __restrict__ cube_at, uint32_t* __restrict__ sbox_at) {
    const uint32_t cube = bb::mul(bb::sqr(x), x), x7 = bb::mul(bb::sqr(cube), x);
    *cube_at = cube;
    *sbox_at = x7;
    return x7;
}

// Row r of the chip's trace (column-major, H_out rows, Montgomery): the r-th smallest witness's 16 inputs re-evaluated, mult = its
// sum mod p, and the RECORDING permutation — the definition (P2Def: ext_rc, int_rc, diag) in plain canonical Montgomery arithmetic, so
// that every stored word is the Montgomery form of the value itself (p2::permute holds scaled representatives, which are not what
// the constraints read). Rows from n on: the zero input, mult 0. The state lives in 16 registers; every store is one word per lane at
// column c, row r: a wave writes 256 contiguous bytes. The round loops stay rolled (the column offset follows the round counter), as in
// p2::permute.
__global__ __launch_bounds__(kBlock) void compress_rows_kernel(const u64* __restrict__ wit, const u64* __restrict__ sum, u64 n, const AirDev* __restrict__ airs,
                                                                P2Def C, size_t H_out, uint32_t* __restrict__ out) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= H_out) return;
    uint32_t s[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0u;
    uint32_t mult = 0u;
    if (r < n) {
        const u64 w = wit[r];
        for (uint32_t j = 0; j < kCompressIn; ++j) {
            const uint32_t v = witness_arg(airs, w, j, stk);
#pragma unroll
            for (int i = 0; i < 16; ++i) s[i] = (uint32_t)i == j ? v : s[i];  // (registers: no run-time index into the state)
        }
        mult = bb::to_monty(sum_residue(sum[r]));
    }
    uint32_t* __restrict__ o = out + r;
    o[0] = mult;
#pragma unroll
    for (int i = 0; i < 16; ++i) o[(size_t)(kP2In + i) * H_out] = s[i];
    p2_external_plain(s);
#pragma unroll 1
    for (int rd = 0; rd < 4; ++rd) {
        uint32_t* __restrict__ c = o + (size_t)(kP2Full + 32 * rd) * H_out;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = p2_sbox_record(bb::add(s[i], C.ext_rc[rd][i]), c + (size_t)i * H_out, c + (size_t)(16 + i) * H_out);
        p2_external_plain(s);
    }
#pragma unroll 1
    for (int k = 0; k < 13; ++k) {
        uint32_t* __restrict__ c = o + (size_t)(kP2Partial + 2 * k) * H_out;
        s[0] = p2_sbox_record(bb::add(s[0], C.int_rc[k]), c, c + H_out);
        uint32_t total = s[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) total = bb::add(total, s[i]);
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = bb::add(total, bb::mul(C.diag[i], s[i]));
    }
#pragma unroll 1
    for (int rd = 4; rd < 8; ++rd) {
        uint32_t* __restrict__ c = o + (size_t)(kP2Full + 32 * rd) * H_out;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = p2_sbox_record(bb::add(s[i], C.ext_rc[rd][i]), c + (size_t)i * H_out, c + (size_t)(16 + i) * H_out);
        p2_external_plain(s);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) o[(size_t)(kP2Out + j) * H_out] = s[j];
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct SysCtx : Scratch {
    Buf small{*this, kStays};  // counters | class loads | AIR table | one witness's arguments
    Buf sums{*this}, table{*this}, keys{*this}, sorted{*this}, temp{*this}, vals{*this}, sorted_vals{*this};
    uint64_t stat_slots = 0, stat_occupied = 0, stat_tables = 0, stat_triples = 0, stat_additions = 0, stat_lds_atomics = 0, stat_global_atomics = 0;
    uint32_t start_log_slots = 0;  // 0: kStartSlots (pw_memory_boundary_set_start_slots)
};
thread_local SysCtx g_sys;

// before any GPU call: false when an interaction on `bus` has not `n_args` arguments
bool bus_arity_is(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, uint32_t n_args) {
    for (size_t a = 0; a < n_airs; ++a) {
        const PwProver* p = airs[a].prover;
        if (!p->logup) continue;
        for (const LogupInteraction& it : p->h_inter)
            if (bb::from_monty(it.bus_monty) == bus && it.n_args != n_args) return false;
    }
    return true;
}

// what the two traces built through a table begin with: the parts of the bus and the triples they hold; small = the walker's head |
// the AIR table, the latter copied (from air_tab: it lives as long as the call)
struct TableWalk { std::vector<Part> parts; std::vector<AirDev> air_tab; u64 triples = 0; WalkHead* d_head = nullptr; AirDev* d_airs = nullptr; };
int begin_table_walk(SysCtx& cx, const PwSegmentAir* airs, size_t n_airs, uint32_t bus, TableWalk* w) {
    PW_TRY(collect_parts(airs, n_airs, bus, w->parts, &w->air_tab));
    for (const Part& part : w->parts) w->triples += ((u64)1 << airs[part.air].log_height) * (part.end - part.begin);
    cx.stat_triples = w->triples;
    PW_TRY(cx.small.ensure(sizeof(WalkHead) + n_airs * sizeof(AirDev)));
    w->d_head = cx.small.as<WalkHead>();
    w->d_airs = (AirDev*)(w->d_head + 1);
    if (n_airs) PW_HIP_TRY(hipMemcpyAsync(w->d_airs, w->air_tab.data(), n_airs * sizeof(AirDev), hipMemcpyHostToDevice, stream()));
    return 0;
}

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" size_t pw_system_traces_scratch_bytes(void) { return g_sys.held(); }
extern "C" size_t pw_system_traces_peak_bytes(void) { return g_sys.peak(); }
extern "C" void pw_system_traces_last_stats(PwSystemTraceStats* out) {
    if (!out) return;
    *out = PwSystemTraceStats{g_sys.stat_slots, g_sys.stat_occupied, g_sys.stat_tables, g_sys.stat_triples, g_sys.stat_additions, g_sys.stat_lds_atomics,
                              g_sys.stat_global_atomics};
}
extern "C" int pw_memory_boundary_set_start_slots(uint32_t log_slots) {
    if (log_slots && (log_slots < 6 || log_slots > 30)) return -1;
    g_sys.start_log_slots = log_slots;
    return 0;
}

extern "C" int pw_program_frequencies(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, uint32_t pc_base, uint32_t pc_step, const uint32_t* d_program,
                                      uint32_t log_h, uint32_t* d_freq_out, uint64_t* n_foreign, PwBusTuple* first_foreign) {
    if (!airs_well_formed(airs, n_airs) || !d_program || !d_freq_out || !n_foreign || !pc_step || log_h > kRowBits || bus >= bb::P) return -1;
    SysCtx& cx = g_sys;
    const ScratchCall call(cx);
    cx.stat_triples = 0;
    *n_foreign = 0;
    const uint32_t table_rows = 1u << log_h;
    std::vector<Part> parts;
    std::vector<AirDev> air_tab;
    PW_TRY(collect_parts(airs, n_airs, bus, parts, &air_tab));
    // small: foreign count, foreign witness, three statistics | AIR table | the witness's multiplicity, arguments
    const size_t off_air = 48, off_args = off_air + n_airs * sizeof(AirDev), small_bytes = off_args + (1 + PW_BUS_MAX_ARGS) * 4;
    PW_TRY(cx.small.ensure(small_bytes));
    PW_TRY(cx.sums.ensure((size_t)table_rows * 8));
    char* base = cx.small.as<char>();
    u64* d_foreign = (u64*)base;
    AirDev* d_airs = (AirDev*)(base + off_air);
    uint32_t* d_args = (uint32_t*)(base + off_args);
    hipStream_t st = stream();
    const u64 foreign0[5] = {0, kEmpty, 0, 0, 0};
    PW_HIP_TRY(hipMemcpyAsync(d_foreign, foreign0, sizeof foreign0, hipMemcpyHostToDevice, st));
    PW_HIP_TRY(hipMemsetAsync(cx.sums.p, 0, (size_t)table_rows * 8, st));
    if (n_airs) PW_HIP_TRY(hipMemcpyAsync(d_airs, air_tab.data(), n_airs * sizeof(AirDev), hipMemcpyHostToDevice, st));
    {
        ScopedKernelTimer timer("program_freq_kernel");
        for (const Part& part : parts) {
            const Walked w = walked(airs[part.air]);
            const uint32_t rows = airs[part.air].log_height >= 16 ? 4u : 1u;
            cx.stat_triples += (uint64_t)w.H * (part.end - part.begin);
            with_fast(w.lp, [&](auto fast) {
                hipLaunchKernelGGL(program_freq_kernel<decltype(fast)::value>, dim3(div_up(w.H, (size_t)kBlock * rows)), dim3(kBlock), 0, st, part.vals, w.H, rows, w.lp,
                                   w.order, part.begin, part.end, (uint32_t)part.air, pc_base, pc_step, d_program, table_rows, cx.sums.as<u64>(), d_foreign);
            });
        }
    }
    hipLaunchKernelGGL(program_freq_finish_kernel, dim3(div_up(table_rows, kBlock)), dim3(kBlock), 0, st, cx.sums.as<u64>(), table_rows, d_freq_out);
    PW_HIP_TRY(hipGetLastError());
    u64 foreign[5];
    PW_HIP_TRY(hipMemcpyAsync(foreign, d_foreign, sizeof foreign, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    *n_foreign = foreign[0];
    cx.stat_additions = foreign[2];
    cx.stat_lds_atomics = foreign[3];
    cx.stat_global_atomics = foreign[4];
    if (foreign[0] && first_foreign) {
        // the tuple at the smallest foreign witness: its own multiplicity, one contribution
        PW_HIP_TRY(hipMemsetAsync(d_args, 0, (1 + PW_BUS_MAX_ARGS) * 4, st));
        hipLaunchKernelGGL(witness_args_kernel, dim3(1), dim3(kBlock), 0, st, (const u64*)(d_foreign + 1), 1u, (u64)1, (const AirDev*)d_airs,
                           (uint32_t)PW_BUS_MAX_ARGS, d_args + 1, d_args);
        PW_HIP_TRY(hipGetLastError());
        uint32_t words[1 + PW_BUS_MAX_ARGS];
        PW_HIP_TRY(hipMemcpyAsync(words, d_args, sizeof words, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        const Witness w = unpack_witness(foreign[1]);
        PwBusTuple& t = *first_foreign;
        memset(&t, 0, sizeof t);
        t.bus = bus;
        t.air = w.air;
        t.interaction = w.inter;
        t.row = w.row;
        t.n_args = airs[t.air].prover->h_inter[t.interaction].n_args;
        for (uint32_t j = 0; j < t.n_args && j < PW_BUS_MAX_ARGS; ++j) t.args[j] = words[1 + j];
        t.net_multiplicity = words[0];
        t.n_contributions = 1;
    }
    return (int)hipGetLastError();
}

extern "C" int pw_memory_boundary_trace(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, size_t table_bytes, uint32_t* d_trace_out,
                                        uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_locations, uint32_t* status) {
    if (!airs_well_formed(airs, n_airs) || !d_trace_out || !log_height || !n_locations || !status || cap_log_height < 1 || cap_log_height > kRowBits ||
        bus >= bb::P)
        return -1;
    if (!bus_arity_is(airs, n_airs, bus, kMemoryArgs)) return -1;
    SysCtx& cx = g_sys;
    const ScratchCall call(cx);
    cx.stat_slots = cx.stat_occupied = cx.stat_tables = cx.stat_triples = 0;
    *log_height = 0;
    *n_locations = 0;
    *status = 0;
    TableWalk tw;
    PW_TRY(begin_table_walk(cx, airs, n_airs, bus, &tw));
    hipStream_t st = stream();
    u64* d_counts = tw.d_head->c.counts;  // occupied | incomplete | written | unused
    AddrTable T{};
    auto walk = [&](auto pass) {
        for (const Part& part : tw.parts) {
            const Walked w = walked(airs[part.air]);
            with_fast(w.lp, [&](auto fast) {
                hipLaunchKernelGGL((boundary_walk_kernel<decltype(fast)::value, decltype(pass)::value>), dim3(div_up(w.H, kBlock)), dim3(kBlock), 0, st, part.vals, w.H,
                                   w.lp, w.order, part.begin, part.end, (uint32_t)part.air, T, &tw.d_head->c.overflow, &tw.d_head->c.flags);
            });
        }
    };
    // pass 1 into tables that grow until one holds the locations (no segment touches more than its triples)
    Grown g;
    PW_TRY(grow_table(
        cx.table, tw.d_head, tw.triples, kSlotBytes, call.bound(table_bytes),
        cx.start_log_slots ? (u64)1 << cx.start_log_slots : kStartSlots, "boundary_table_clear",
        [&](u64* tb, const TableRule& rule) -> int {
            const u64 slots = rule.mask + 1;
            T = AddrTable{TableView{rule, tb, nullptr}, tb + slots, tb + 2 * slots, tb + 3 * slots, tb + 4 * slots};
            PW_HIP_TRY(hipMemsetAsync(tb, 0xFF, 4 * slots * 8, st));
            PW_HIP_TRY(hipMemsetAsync(tb + 4 * slots, 0, slots * 8, st));
            return 0;
        },
        [&] {
            ScopedKernelTimer timer("boundary_walk_kernel");
            walk(std::integral_constant<int, 1>{});
        },
        [&] { hipLaunchKernelGGL(boundary_compact_kernel, dim3(div_up(T.v.mask + 1, kBlock)), dim3(kBlock), 0, st, T, (u64*)nullptr, (u64)0, d_counts); }, &g));
    cx.stat_tables = g.tables;
    if (g.no_table || g.overflowed()) {
        *status = 2;
        return (int)hipGetLastError();
    }
    const u64 n = g.c.counts[0], slots = g.slots;
    cx.stat_slots = slots;
    cx.stat_occupied = n;
    *n_locations = n;
    const uint32_t lh = ceil_log2_at_least_1(n);
    *log_height = lh;
    if (g.c.flags & kFlagMagnitude) {
        *status = 3;
        return (int)hipGetLastError();
    }
    if (g.c.counts[1]) {
        *status = 4;
        return (int)hipGetLastError();
    }
    if (lh > cap_log_height) {
        *status = 1;
        return (int)hipGetLastError();
    }
    {
        ScopedKernelTimer timer("boundary_witness_kernel");
        walk(std::integral_constant<int, 2>{});
    }
    const size_t H_out = (size_t)1 << lh;
    if (n) {
        PW_TRY(cx.keys.ensure(n * 8));
        PW_TRY(cx.sorted.ensure(n * 8));
        hipLaunchKernelGGL(boundary_compact_kernel, dim3(div_up(slots, kBlock)), dim3(kBlock), 0, st, T, cx.keys.as<u64>(), n, d_counts);
        PW_HIP_TRY(hipGetLastError());
        ScopedKernelTimer timer("boundary_sort");
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, cx.keys.as<u64>(), cx.sorted.as<u64>(), (size_t)n, 0u, 64u, st); }));
    }
    {
        ScopedKernelTimer timer("boundary_rows_kernel");
        hipLaunchKernelGGL(boundary_rows_kernel, dim3(div_up(H_out, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.sorted.p, n, T, (const AirDev*)tw.d_airs, H_out, d_trace_out);
    }
    PW_HIP_TRY(hipGetLastError());
    PW_HIP_TRY(hipStreamSynchronize(st));
    return (int)hipGetLastError();
}

extern "C" int pw_poseidon2_compress_trace(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, size_t table_bytes, uint32_t start_log_slots,
                                           uint32_t* d_trace_out, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_rows, uint32_t* status) {
    if (!airs_well_formed(airs, n_airs) || !d_trace_out || !log_height || !n_rows || !status || cap_log_height < 1 || cap_log_height > kRowBits ||
        bus >= bb::P || (start_log_slots && (start_log_slots < 6 || start_log_slots > 30)))
        return -1;
    if (!bus_arity_is(airs, n_airs, bus, kCompressArgs)) return -1;
    SysCtx& cx = g_sys;
    const ScratchCall call(cx);
    cx.stat_slots = cx.stat_occupied = cx.stat_tables = cx.stat_triples = 0;
    *log_height = 0;
    *n_rows = 0;
    *status = 0;
    TableWalk tw;
    PW_TRY(begin_table_walk(cx, airs, n_airs, bus, &tw));
    hipStream_t st = stream();
    u64* d_counts = tw.d_head->c.counts;  // occupied | unused | written | unused

    // the definition of the installed permutation, and the fingerprint's challenges: a fixed splitmix64 stream — nothing written
    // depends on them short of a collision, which costs a key its row and leaves its tuple unbalanced on the bus
    P2Def def;
    {
        const p2::Params& hp = poseidon2_params_host();
        memcpy(def.ext_rc, hp.ext_rc, sizeof def.ext_rc);
        memcpy(def.int_rc, hp.int_rc, sizeof def.int_rc);
        memcpy(def.diag, hp.diag, sizeof def.diag);
    }
    P2Key key;
    {
        uint64_t sm = 0x70325f636f6d7072ull;
        key.al = challenge(sm);
        const bb::Ext bl = challenge(sm);
        key.blpow[0] = bb::ext_one();
        for (uint32_t j = 1; j <= kCompressIn; ++j) key.blpow[j] = bb::ext_mul(key.blpow[j - 1], bl);
    }

    P2Table T{};
    Grown g;
    PW_TRY(grow_table(
        cx.table, tw.d_head, tw.triples, kP2SlotBytes, call.bound(table_bytes),
        start_log_slots ? (u64)1 << start_log_slots : kStartSlots, "compress_table_clear",
        [&](u64* tb, const TableRule& rule) -> int {
            const u64 slots = rule.mask + 1;
            T = P2Table{TableView{rule, tb, tb + slots}, tb + 2 * slots, tb + 3 * slots};
            PW_HIP_TRY(hipMemsetAsync(tb, 0xFF, 2 * slots * 8, st));
            PW_HIP_TRY(hipMemsetAsync(tb + 2 * slots, 0, slots * 8, st));
            PW_HIP_TRY(hipMemsetAsync(tb + 3 * slots, 0xFF, slots * 8, st));
            return 0;
        },
        [&] {
            ScopedKernelTimer timer("compress_tally_kernel");
            for (const Part& part : tw.parts) {
                const Walked w = walked(airs[part.air]);
                with_fast(w.lp, [&](auto fast) {
                    hipLaunchKernelGGL(compress_tally_kernel<decltype(fast)::value>, dim3(div_up(w.H, kBlock)), dim3(kBlock), 0, st, part.vals, w.H, w.lp, w.order,
                                       part.begin, part.end, (uint32_t)part.air, key, T, &tw.d_head->c.overflow);
                });
            }
        },
        [&] {
            hipLaunchKernelGGL(compress_compact_kernel, dim3(div_up(T.v.mask + 1, kBlock)), dim3(kBlock), 0, st, T, (u64*)nullptr, (u64*)nullptr, (u64)0, d_counts);
        },
        &g));
    cx.stat_tables = g.tables;
    if (g.no_table || g.overflowed()) {
        *status = 2;
        return (int)hipGetLastError();
    }
    const u64 n = g.c.counts[0], slots = g.slots;
    cx.stat_slots = slots;
    cx.stat_occupied = n;
    *n_rows = n;
    const uint32_t lh = ceil_log2_at_least_1(n);
    *log_height = lh;
    if (lh > cap_log_height) {
        *status = 1;
        return (int)hipGetLastError();
    }
    const size_t H_out = (size_t)1 << lh;
    if (n) {
        PW_TRY(cx.keys.ensure(n * 8));
        PW_TRY(cx.vals.ensure(n * 8));
        PW_TRY(cx.sorted.ensure(n * 8));
        PW_TRY(cx.sorted_vals.ensure(n * 8));
        hipLaunchKernelGGL(compress_compact_kernel, dim3(div_up(slots, kBlock)), dim3(kBlock), 0, st, T, cx.keys.as<u64>(), cx.vals.as<u64>(), n, d_counts);
        PW_HIP_TRY(hipGetLastError());
        ScopedKernelTimer timer("compress_sort");
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::radix_sort_pairs(t, b, cx.keys.as<u64>(), cx.sorted.as<u64>(), cx.vals.as<u64>(), cx.sorted_vals.as<u64>(), (size_t)n, 0u, 64u, st);
        }));
    }
    {
        ScopedKernelTimer timer("compress_rows_kernel");
        hipLaunchKernelGGL(compress_rows_kernel, dim3(div_up(H_out, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.sorted.p, (const u64*)cx.sorted_vals.p, n,
                           (const AirDev*)tw.d_airs, def, H_out, d_trace_out);
    }
    PW_HIP_TRY(hipGetLastError());
    PW_HIP_TRY(hipStreamSynchronize(st));
    return (int)hipGetLastError();
}
