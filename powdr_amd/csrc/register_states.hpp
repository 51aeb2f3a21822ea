// The states of an execution from its traces — pcs, requested registers and time keys in time order: the stage
// pw_execution_states_from_traces (execution_states.hip) and pw_apc_calls_from_traces_registers (apc_calls.hip) share. Positions,
// time keys and pcs are time_index::rows_in_time_order unchanged; the registers come from the memory bus:
//   walk    execution_states_walk_kernel     one lane per row of every AIR on the memory bus evaluates its interactions as the boundary
//                                            walk does. A send to a requested register is appended as (table row << 32 | t, word,
//                                            witness): one counter add per wave and interaction, the lanes' places by their rank among
//                                            the senders. A receive lowers the register's (previous ts << 32 | word): the lanes of a wave
//                                            merge per distinct register (wave_min), and a relaxed load spares the atomic that would lose
//   sort    a radix sort of the sends by (table row, t). The places the walk gave depend on the order of arrival; the sorted keys do
//           not — two sends with one key are status 8 — and the payload is read through the sorted index, so nothing that leaves does
//   place   execution_states_place_kernel    one lane per sorted send: p = #{j : ts_j <= t} by binary search over the sorted time keys; a
//                                            send is kept iff its successor has another register or another p (the largest t of an
//                                            instruction wins); an exclusive scan and execution_states_keep_kernel compact (row, p, word)
//   fill    execution_states_fill_kernel     one workgroup per (register, tile of kTile table words): a binary search over the kept
//                                            sends finds the one that covers the tile's first state, the tile's own sends are scattered
//                                            into LDS and max-scanned, every lane stores 4 consecutive states as one 16-byte store
// Not part of the C ABI.
#pragma once
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

namespace pw {
namespace register_states {

using namespace bus;

constexpr uint32_t kMemoryArgs = 7;    // as, ptr, four data words, timestamp
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr uint32_t kTile = 4 * kBlock;  // table words a workgroup of the fill writes
constexpr int kMergeRounds = 4;        // distinct registers a wave merges before its lanes fall back to one atomic each
constexpr uint32_t kMaxRows = 65535;   // table rows (the fill's grid)

namespace {

// the table row of register reg, or kNoRow: sorted[] ascending, row_of[] the rows in that order
__device__ __forceinline__ uint32_t row_of_register(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ row_of, uint32_t n, uint32_t reg) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < reg) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && sorted[lo] == reg ? row_of[lo] : kNoRow;
}

__device__ __forceinline__ void lower_first(u64* __restrict__ first, uint32_t row, u64 v) {
    if (__atomic_load_n(first + row, __ATOMIC_RELAXED) > v) atomicMin(first + row, v);
}

// counters: [0] sends appended | [1] the smallest witness of a register tuple that is none
// Every loop is wave-uniform (a lane past the last row carries no tuple), so that the lanes of a wave can merge.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void execution_states_walk_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                                        uint32_t begin, uint32_t end, uint32_t air, uint32_t reg_as, uint32_t ptr_step,
                                                                        const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ row_of, uint32_t n_rows,
                                                                        u64* __restrict__ skey, uint32_t* __restrict__ sword, u64* __restrict__ swit, u64 cap,
                                                                        u64* __restrict__ first, u64* __restrict__ counters) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    u64 bad = kEmpty;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t idx = order[i];
        const LogupInteraction it = lp.d_inter[idx];
        uint32_t row = kNoRow, word = 0, t = 0;
        int32_t cm = 0;
        if (r < H) {
            const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
            if (mu != 0u && bb::from_monty(eval_span<FAST>(lp, it.first_span + 1, m, H, r, stk)) == reg_as) {
                cm = bb::centred(bb::from_monty(mu));
                const uint32_t ptr = bb::from_monty(eval_span<FAST>(lp, it.first_span + 2, m, H, r, stk));
                bool ok = (cm == 1 || cm == -1) && ptr % ptr_step == 0u;
                if (ok) {
                    row = row_of_register(sorted, row_of, n_rows, ptr / ptr_step);
                    if (row != kNoRow) {
                        for (uint32_t j = 0; j < 4; ++j) {
                            const uint32_t d = bb::from_monty(eval_span<FAST>(lp, it.first_span + 3 + j, m, H, r, stk));
                            ok = ok && d < 256u;
                            word |= (d & 0xffu) << (8u * j);
                        }
                        t = bb::from_monty(eval_span<FAST>(lp, it.first_span + kMemoryArgs, m, H, r, stk));
                    }
                }
                if (!ok) {
                    const u64 w = pack_witness(air, idx, r);
                    bad = w < bad ? w : bad;
                    row = kNoRow;
                }
            }
        }
        const bool send = row != kNoRow && cm == 1, recv = row != kNoRow && cm == -1;
        const u64 senders = __builtin_amdgcn_ballot_w64(send);
        if (senders) {
            const int leader = __builtin_ctzll(senders);
            u64 base = 0;
            if ((int)lane == leader) base = atomicAdd(counters, (u64)__builtin_popcountll(senders));
            base = __shfl(base, leader, 64);
            const u64 at = base + (u64)__builtin_popcountll(senders & ((1ull << lane) - 1ull));
            if (send && at < cap) {  // (cap holds every interaction of every row)
                skey[at] = ((u64)row << 32) | (u64)t;
                sword[at] = word;
                swit[at] = pack_witness(air, idx, r);
            }
        }
        const u64 v = recv ? ((u64)t << 32) | (u64)word : kEmpty;
        u64 todo = __builtin_amdgcn_ballot_w64(recv);
        for (int round = 0; round < kMergeRounds && todo; ++round) {
            const int leader = __builtin_ctzll(todo);
            const uint32_t key = (uint32_t)__shfl((int)row, leader, 64);
            const bool mine = recv && row == key;
            const u64 lowest = wave_min(mine ? v : kEmpty);
            if ((int)lane == leader) lower_first(first, key, lowest);
            todo &= ~__builtin_amdgcn_ballot_w64(mine);
        }
        if ((todo >> lane) & 1ull) lower_first(first, row, v);  // (a wave with many distinct registers)
    }
    if (__builtin_amdgcn_ballot_w64(bad != kEmpty)) {  // (never on honest traces)
        const u64 w = wave_min(bad);
        if (lane == 0u) atomicMin(counters + 1, w);
    }
}

// #{ j < N : the timestamp of position j <= t } (one segment: the low words of the time keys ascend)
__device__ __forceinline__ uint32_t position_of(const u64* __restrict__ tkey_s, u64 N, uint32_t t) {
    u64 lo = 0, hi = N;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((uint32_t)tkey_s[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return (uint32_t)lo;
}

__global__ __launch_bounds__(kBlock) void execution_states_place_kernel(const u64* __restrict__ skey_s, const uint32_t* __restrict__ idx_s, const u64* __restrict__ swit, u64 n,
                                                                         const u64* __restrict__ tkey_s, u64 N, uint32_t* __restrict__ pos, uint32_t* __restrict__ keep,
                                                                         u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    u64 bad = kEmpty;
    if (i < n) {
        const u64 k = skey_s[i];
        const uint32_t p = position_of(tkey_s, N, (uint32_t)k);
        bool twice = i && skey_s[i - 1] == k, kept = true;
        if (i + 1 < n) {
            const u64 next = skey_s[i + 1];
            twice = twice || next == k;
            kept = (next >> 32) != (k >> 32) || position_of(tkey_s, N, (uint32_t)next) != p;
        }
        pos[i] = p;
        keep[i] = kept ? 1u : 0u;
        if (twice || p == 0u) bad = swit[idx_s[i]];  // one (register, timestamp) twice; a send before the first instruction
    }
    if (__builtin_amdgcn_ballot_w64(bad != kEmpty)) {
        const u64 w = wave_min(bad);
        if ((threadIdx.x & 63u) == 0u) atomicMin(counters + 1, w);
    }
}

__global__ __launch_bounds__(kBlock) void execution_states_keep_kernel(const u64* __restrict__ skey_s, const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ sword,
                                                                        const uint32_t* __restrict__ pos, const uint32_t* __restrict__ keep, const uint32_t* __restrict__ off,
                                                                        u64 n, u64* __restrict__ kp, uint32_t* __restrict__ kw) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n || !keep[i]) return;
    kp[off[i]] = (skey_s[i] & ~0xffffffffull) | (u64)pos[i];
    kw[off[i]] = sword[idx_s[i]];
}

// Row blockIdx.y of the table, out[row * n_states + s] for the states s whose words lie in the tile: the table words
// [row * n_states rounded down to a multiple of 4, + kTile * blockIdx.x ...), so that every lane's 4 words are one aligned 16 bytes
// whatever the row's first word is. kp: the kept sends (row << 32 | p) ascending, kw their words; at0[row]: the value at state 0.
__global__ __launch_bounds__(kBlock) void execution_states_fill_kernel(const u64* __restrict__ kp, const uint32_t* __restrict__ kw, u64 n_kept,
                                                                        const uint32_t* __restrict__ at0, u64 n_states, uint32_t* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) int32_t last[kTile];  // per word of the tile: the tile's send placed at that state (from e0), -1 = none
    __shared__ int32_t wave_last[kWaves];
    const uint32_t row = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u64 o = (u64)row * n_states;
    const long long s_first = (long long)blockIdx.x * kTile - (long long)(o & 3ull);  // the state of the tile's first word (below 0: the row before)
    if (s_first >= (long long)n_states) return;
    const u64 s_lo = s_first < 0 ? 0ull : (u64)s_first;
    const u64 s_end = (u64)(s_first + kTile) < n_states ? (u64)(s_first + kTile) : n_states;
    // e0 = the kept sends at or before (row, s_lo): the last of them covers s_lo if it is this row's
    const u64 probe = ((u64)row << 32) | s_lo;
    u64 lo = 0, hi = n_kept;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (kp[mid] <= probe) lo = mid + 1;
        else hi = mid;
    }
    const u64 e0 = lo;
    const uint32_t before = e0 && (kp[e0 - 1] >> 32) == row ? kw[e0 - 1] : at0[row];
    for (uint32_t k = tid; k < kTile; k += kBlock) last[k] = -1;
    __syncthreads();
    for (u64 e = e0 + tid; e < n_kept; e += kBlock) {  // (at most one send per state: kTile of them lie in the tile)
        const u64 v = kp[e];
        if ((v >> 32) != row || (v & 0xffffffffull) >= s_end) break;
        last[(long long)(v & 0xffffffffull) - s_first] = (int32_t)(e - e0);
    }
    __syncthreads();
    const int4 mine = *reinterpret_cast<const int4*>(&last[4u * tid]);
    int32_t a[4] = {mine.x, mine.y, mine.z, mine.w};
#pragma unroll
    for (int j = 1; j < 4; ++j) a[j] = a[j] > a[j - 1] ? a[j] : a[j - 1];
    int32_t incl = a[3];  // the running maximum over the lanes before and this one
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t other = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl = other > incl ? other : incl;
    }
    if (lane == 63u) wave_last[wave] = incl;
    int32_t prefix = __shfl_up(incl, 1, 64);
    if (lane == 0u) prefix = -1;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w) prefix = wave_last[w] > prefix ? wave_last[w] : prefix;
    uint32_t val[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int32_t e = a[j] > prefix ? a[j] : prefix;
        val[j] = e < 0 ? before : kw[e0 + (u64)e];
    }
    const long long s0 = s_first + 4ll * tid;
    if (s0 >= 0 && s0 + 4 <= (long long)n_states) {
        *reinterpret_cast<uint4*>(out + o + (u64)s0) = make_uint4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (s0 + j >= 0 && s0 + j < (long long)n_states) out[o + (u64)(s0 + j)] = val[j];
    }
}

}  // namespace

// what the two entry points take of the traces
struct Args {
    const PwSegmentAir* airs;
    const uint32_t* segment_of_air;
    size_t n_airs;
    uint32_t bridge_bus, memory_bus, final_pc, reg_as, ptr_step;
};

// false = -1: a NULL AIR list, a bus id >= p, reg_ptr_step == 0, two segment numbers, a malformed AIR list, an interaction on the
// bridge with an arity other than 2 or on the memory bus with one other than 7. *B = the bridge's AIRs and rows, *slots = the
// interactions on the memory bus times their AIRs' rows: no walk appends more sends.
inline bool args_ok(const Args& a, time_index::Bridge* B, u64* slots) {
    if (a.bridge_bus >= bb::P || a.memory_bus >= bb::P || !a.ptr_step || !time_index::one_segment(a.segment_of_air, a.n_airs) || !airs_well_formed(a.airs, a.n_airs) ||
        !time_index::bridge_of(a.airs, a.n_airs, a.bridge_bus, B) || B->M + 1 >= ((u64)1 << 32))
        return false;
    bool seven_args = true;
    *slots = 0;
    for (size_t k = 0; k < a.n_airs; ++k) *slots += (u64)interactions_on(a.airs[k].prover, a.memory_bus, kMemoryArgs, &seven_args) << a.airs[k].log_height;
    return seven_args && *slots < ((u64)1 << 32);
}

// false = -1: a NULL list, more than kMaxRows rows, a register whose pointer is no field element, one register twice
inline bool registers_ok(const uint32_t* regs, size_t n, uint32_t ptr_step) {
    if ((!regs && n) || n > kMaxRows) return false;
    std::vector<uint32_t> s(regs, regs + n);
    std::sort(s.begin(), s.end());
    if (std::adjacent_find(s.begin(), s.end()) != s.end()) return false;
    return s.empty() || s.back() <= (bb::P - 1u) / ptr_step;
}

// the scratch of the stage: everything but the three arrays that leave
struct Ctx : Scratch {
    Ctx() = default;  // a context of its own (execution_states.hip)
    explicit Ctx(Scratch& owner) : Scratch(owner) {}  // a stage of another pipeline's (apc_calls.hip)
    time_index::Stage index{*this};
    Buf temp{*this}, small{*this}, skey{*this}, skey_s{*this}, sidx{*this}, sidx_s{*this}, sword{*this}, swit{*this}, pos{*this}, keep{*this}, off{*this}, kp{*this},
        kw{*this};
    uint64_t sends = 0, kept = 0;
    void reset_stats() override { sends = kept = 0; }
};

// Bytes that always suffice, before a row is read: the three arrays that leave; the index stage's 32 bytes per bridge row; per slot
// 28 while the walk appends (key, word, witness, index), 12 sorted, 12 placed (position, flag, offset) and 12 kept; the larger
// temporary storage; the small tables per register.
inline size_t bytes_needed(u64 M, u64 slots, u64 n_rows) {
    const size_t temp = std::max({M ? time_index::sort_pairs_temp(M) : 16, slots ? time_index::sort_pairs_temp(slots) : 16,
                                  slots ? time_index::scan_temp((uint32_t*)nullptr, slots) : 16});
    return 4096 + (size_t)(M + 1) * 4 * (n_rows + 1) + (size_t)M * 8 + (size_t)M * 32 + (size_t)slots * 64 + temp + (size_t)n_rows * 32;
}

// The states of the traces into pcs[N + 1], table[n_rows x (N + 1)] (row k = register regs[k]) and keys[N]; *N_out = N. B, slots: of
// args_ok. initial: NULL or one word per row. *status = 7, 4, 8, 9 or 10 with *info where there are none; then nothing is valid.
// The three arrays are Scratch::Buf of the caller's context, or the plain DeviceBuf of a handle under construction, whose bytes are
// then the scratch's `extra`. The caller releases cx.
template <class Out>
inline int states_from_traces(const Args& a, const std::vector<uint32_t>& regs, const uint32_t* initial, const time_index::Bridge& B, u64 slots, Ctx& cx, Out& pcs, Out& table, Out& keys,
                              u64* N_out, uint32_t* status, uint64_t* info) {
    hipStream_t st = stream();
    const uint32_t n_rows = (uint32_t)regs.size();
    cx.sends = cx.kept = 0;
    u64 N = 0;
    PW_TRY(time_index::open(a.airs, a.segment_of_air, a.n_airs, a.bridge_bus, B, cx.index, cx.temp,
                            time_index::Names{"execution_states_index", "execution_states_sort_time", "execution_states_time"}, &N, status, info));
    if (*status) return (int)hipGetLastError();
    *N_out = N;
    const u64 n_states = N + 1;
    PW_TRY(pcs.ensure(n_states * 4));
    PW_TRY(keys.ensure(std::max<u64>(N, 1) * 8));
    PW_TRY(table.ensure(std::max<u64>((u64)n_rows * n_states, 1) * 4));
    if (!std::is_base_of<Scratch::Buf, Out>::value) cx.set_extra(pcs.bytes + keys.bytes + table.bytes);
    if (N) {
        PW_HIP_TRY(hipMemcpyAsync(pcs.p, cx.index.pc_t.p, N * 4, hipMemcpyDeviceToDevice, st));
        PW_HIP_TRY(hipMemcpyAsync(keys.p, cx.index.tkey_s.p, N * 8, hipMemcpyDeviceToDevice, st));
    }
    PW_HIP_TRY(hipMemcpyAsync(pcs.template as<uint32_t>() + N, &a.final_pc, 4, hipMemcpyHostToDevice, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    cx.index.release();
    if (!n_rows) return (int)hipGetLastError();

    // small: counters (8 u64) | first (n_rows u64) | at0 (n_rows u32) | sorted registers | their rows
    std::vector<uint32_t> by_reg(n_rows);
    for (uint32_t k = 0; k < n_rows; ++k) by_reg[k] = k;
    std::sort(by_reg.begin(), by_reg.end(), [&](uint32_t x, uint32_t y) { return regs[x] < regs[y]; });
    std::vector<u64> head(8 + n_rows, kEmpty);
    head[0] = 0;
    std::vector<uint32_t> tail(3 * (size_t)n_rows, 0u);
    for (uint32_t k = 0; k < n_rows; ++k) {
        tail[n_rows + k] = regs[by_reg[k]];
        tail[2 * (size_t)n_rows + k] = by_reg[k];
    }
    const size_t head_bytes = head.size() * 8;
    PW_TRY(cx.small.ensure(head_bytes + tail.size() * 4));
    char* sm = cx.small.as<char>();
    u64* d_counters = (u64*)sm;
    u64* d_first = d_counters + 8;
    uint32_t* d_at0 = (uint32_t*)(sm + head_bytes);
    const uint32_t *d_sorted = d_at0 + n_rows, *d_row_of = d_sorted + n_rows;
    PW_HIP_TRY(hipMemcpyAsync(sm, head.data(), head_bytes, hipMemcpyHostToDevice, st));
    PW_HIP_TRY(hipMemcpyAsync(d_at0, tail.data(), tail.size() * 4, hipMemcpyHostToDevice, st));
    if (slots) {
        ScopedKernelTimer timer("execution_states_walk");
        std::vector<Part> parts;
        PW_TRY(collect_parts(a.airs, a.n_airs, a.memory_bus, parts, nullptr));
        PW_TRY(cx.skey.ensure(slots * 8));
        PW_TRY(cx.sword.ensure(slots * 4));
        PW_TRY(cx.swit.ensure(slots * 8));
        for (const Part& part : parts) {
            const Walked w = walked(a.airs[part.air]);
            with_fast(w.lp, [&](auto fast) {
                hipLaunchKernelGGL(execution_states_walk_kernel<decltype(fast)::value>, dim3(div_up(w.H, kBlock)), dim3(kBlock), 0, st, part.vals, w.H, w.lp, w.order,
                                   part.begin, part.end, (uint32_t)part.air, a.reg_as, a.ptr_step, d_sorted, d_row_of, n_rows, cx.skey.as<u64>(), cx.sword.as<uint32_t>(),
                                   cx.swit.as<u64>(), slots, d_first, d_counters);
            });
        }
        PW_HIP_TRY(hipGetLastError());
    }
    std::vector<u64> got(8 + n_rows);
    PW_HIP_TRY(hipMemcpyAsync(got.data(), sm, head_bytes, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    const u64 n_sends = got[0];
    if (n_sends > slots) return (int)hipErrorInvalidValue;  // (cannot happen: more sends than interactions)
    cx.sends = n_sends;
    u64 n_kept = 0;
    if (n_sends) {
        {
            ScopedKernelTimer timer("execution_states_sort");
            PW_TRY(cx.skey_s.ensure(n_sends * 8));
            PW_TRY(cx.sidx.ensure(n_sends * 4));
            PW_TRY(cx.sidx_s.ensure(n_sends * 4));
            hipLaunchKernelGGL(time_index::empirical_iota_kernel, dim3(div_up(n_sends, kBlock)), dim3(kBlock), 0, st, cx.sidx.as<uint32_t>(), n_sends);
            PW_HIP_TRY(hipGetLastError());
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                return rocprim::radix_sort_pairs(t, b, cx.skey.as<u64>(), cx.skey_s.as<u64>(), cx.sidx.as<uint32_t>(), cx.sidx_s.as<uint32_t>(), (size_t)n_sends, 0u, 64u, st);
            }));
        }
        {
            ScopedKernelTimer timer("execution_states_place");
            PW_TRY(cx.pos.ensure(n_sends * 4));
            PW_TRY(cx.keep.ensure(n_sends * 4));
            PW_TRY(cx.off.ensure(n_sends * 4));
            hipLaunchKernelGGL(execution_states_place_kernel, dim3(div_up(n_sends, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.skey_s.p, (const uint32_t*)cx.sidx_s.p,
                               (const u64*)cx.swit.p, n_sends, (const u64*)keys.p, N, cx.pos.as<uint32_t>(), cx.keep.as<uint32_t>(), d_counters);
            PW_HIP_TRY(hipGetLastError());
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                return rocprim::exclusive_scan(t, b, cx.keep.as<uint32_t>(), cx.off.as<uint32_t>(), 0u, (size_t)n_sends, rocprim::plus<uint32_t>(), st);
            }));
            uint32_t last[2] = {0, 0};
            PW_HIP_TRY(hipMemcpyAsync(&last[0], cx.off.as<uint32_t>() + (n_sends - 1), 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipMemcpyAsync(&last[1], cx.keep.as<uint32_t>() + (n_sends - 1), 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipMemcpyAsync(got.data(), sm, 16, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            n_kept = (u64)last[0] + last[1];
        }
    }
    if (got[1] != kEmpty) {
        *status = 8;
        *info = got[1];
        return (int)hipGetLastError();
    }
    // the value at state 0: what the receive with the smallest previous timestamp carried, or the caller's word
    std::vector<uint32_t> at0(n_rows);
    u64 none = kEmpty, contradicted = kEmpty;
    for (uint32_t k = 0; k < n_rows; ++k) {
        const u64 f = got[8 + k];
        if (f == kEmpty && !initial) none = std::min<u64>(none, regs[k]);
        if (f != kEmpty && initial && initial[k] != (uint32_t)f) contradicted = std::min<u64>(contradicted, regs[k]);
        at0[k] = initial ? initial[k] : (uint32_t)f;
    }
    if (none != kEmpty || contradicted != kEmpty) {
        *status = none != kEmpty ? 9 : 10;
        *info = none != kEmpty ? none : contradicted;
        return (int)hipGetLastError();
    }
    PW_HIP_TRY(hipMemcpyAsync(d_at0, at0.data(), (size_t)n_rows * 4, hipMemcpyHostToDevice, st));
    if (n_kept) {
        ScopedKernelTimer timer("execution_states_place");
        PW_TRY(cx.kp.ensure(n_kept * 8));
        PW_TRY(cx.kw.ensure(n_kept * 4));
        hipLaunchKernelGGL(execution_states_keep_kernel, dim3(div_up(n_sends, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.skey_s.p, (const uint32_t*)cx.sidx_s.p,
                           (const uint32_t*)cx.sword.p, (const uint32_t*)cx.pos.p, (const uint32_t*)cx.keep.p, (const uint32_t*)cx.off.p, n_sends, cx.kp.as<u64>(),
                           cx.kw.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
    }
    cx.kept = n_kept;
    {
        ScopedKernelTimer timer("execution_states_fill");
        const u64 tiles = div_up(n_states + 3, kTile);
        hipLaunchKernelGGL(execution_states_fill_kernel, dim3((unsigned)tiles, n_rows), dim3(kBlock), 0, st, (const u64*)cx.kp.p, (const uint32_t*)cx.kw.p, n_kept,
                           (const uint32_t*)d_at0, n_states, table.template as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
    }
    PW_HIP_TRY(hipStreamSynchronize(st));  // (at0 is a local)
    return (int)hipGetLastError();
}

}  // namespace register_states
}  // namespace pw
