// The executed rows of a segment in time order — the stage the empirical-constraint detector (empirical.hip) and the
// superblock detector (execution_blocks.hip, §5q) share: ONE copy of the bridge evaluation, the time sort and the block-table lookup.
//   index      empirical_index_kernel     one lane per (AIR, row) evaluates the bridge exactly as the bus check does: an active row
//                                         writes its time key (segment << 32 | timestamp) and pc at its GLOBAL row number, a padding
//                                         row the key ~0 — no compaction, so nothing depends on an order of arrival; a radix sort of
//                                         (time key, row number) puts the active rows first, in time order
//   time       empirical_time_kernel      neighbours with one key (status 4), the number of active rows, the pcs in time order
// Not part of the C ABI.
#pragma once
#include "scratch.hpp"
#include "prover_internal.hpp"

#include <rocprim/rocprim.hpp>

namespace pw {
namespace time_index {

using namespace bus;

constexpr uint32_t kNoPc = 0xffffffffu;

namespace {

// counters: [0] active rows | [1] smallest (air << 32 | row) with bad multiplicities | [2] smallest duplicate key | [3 ..] the caller's
template <bool FAST>
__global__ __launch_bounds__(kBlock) void empirical_index_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                                  uint32_t begin, uint32_t end, uint32_t air, uint32_t segment, u64 g0,
                                                                  u64* __restrict__ tkey, uint32_t* __restrict__ pcs, u64* __restrict__ counters) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    bool active = false, bad = false;
    uint32_t n_recv = 0, pc = 0, ts = 0;
    if (r < H) {
        for (uint32_t i = begin; i < end; ++i) {
            const uint32_t idx = order[i];
            const LogupInteraction it = lp.d_inter[idx];
            const uint32_t mu = eval_span<FAST>(lp, it.first_span, m, H, r, stk);
            if (mu == 0u) continue;
            active = true;
            const int32_t cm = bb::centred(bb::from_monty(mu));
            if (cm == -1) {
                if (n_recv++ == 0u) {
                    pc = bb::from_monty(eval_span<FAST>(lp, it.first_span + 1, m, H, r, stk));
                    ts = bb::from_monty(eval_span<FAST>(lp, it.first_span + 2, m, H, r, stk));
                }
            } else if (cm != 1) {
                bad = true;
            }
        }
        bad = active && (bad || n_recv != 1u);
        const bool ok = active && !bad;
        tkey[g0 + r] = ok ? ((u64)segment << 32) | (u64)ts : kEmpty;
        pcs[g0 + r] = ok ? pc : kNoPc;
    }
    if (__builtin_amdgcn_ballot_w64(bad)) {  // (never on honest traces)
        const u64 w = wave_min(bad ? ((u64)air << 32) | (u64)r : kEmpty);
        if ((threadIdx.x & 63u) == 0u) atomicMin(counters + 1, w);
    }
}

__global__ __launch_bounds__(kBlock) void empirical_iota_kernel(uint32_t* __restrict__ out, u64 n) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i < n) out[i] = (uint32_t)i;
}

// over the rows in time order: the pcs in that order, the number of active rows (the padding keys sort last), a key held twice
__global__ __launch_bounds__(kBlock) void empirical_time_kernel(const u64* __restrict__ tkey_s, const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ pcs,
                                                                 u64 M, uint32_t* __restrict__ pc_t, u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= M) return;
    const u64 k = tkey_s[i];
    pc_t[i] = pcs[idx_s[i]];
    if (k == kEmpty) return;
    const u64 next = i + 1 < M ? tkey_s[i + 1] : kEmpty;
    if (next == kEmpty) counters[0] = i + 1;
    else if (next == k) atomicMin(counters + 2, k);
}

// the block that holds pc as one of its instructions: its index and the instruction's, or false
__device__ __forceinline__ bool find_block(const PwBasicBlock* __restrict__ blocks, uint32_t n_blocks, uint32_t pc_step, uint32_t pc, uint32_t* b, uint32_t* k) {
    uint32_t lo = 0, hi = n_blocks;  // the last block with start_pc <= pc
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (blocks[mid].start_pc <= pc) lo = mid + 1;
        else hi = mid;
    }
    if (!lo) return false;
    const PwBasicBlock B = blocks[lo - 1];
    const uint32_t d = pc - B.start_pc;
    if (d % pc_step != 0u || d / pc_step >= B.n_instructions) return false;
    *b = lo - 1;
    *k = d / pc_step;
    return true;
}

}  // namespace

inline size_t sort_pairs_temp(size_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (u64*)nullptr, (u64*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, 64u, stream());
    return std::max<size_t>(bytes, 16);
}

// The temporary storage of an exclusive scan that adds up n words read through `in`. rocPRIM sizes it by the input iterator's type as
// well as by n, so a "bytes that always suffice" formula asks with the iterator its pipeline scans with: a plain pointer in
// register_states.hpp, a transform iterator over bytes in apc_sources.hip.
template <class In>
inline size_t scan_temp(In in, size_t n) {
    size_t bytes = 0;
    (void)rocprim::exclusive_scan(nullptr, bytes, in, (uint32_t*)nullptr, 0u, n, rocprim::plus<uint32_t>(), stream());
    return std::max<size_t>(bytes, 16);
}

// -1 where the block table is unsorted, overlapping or has a zero count
inline bool blocks_well_formed(const PwBasicBlock* blocks, size_t n_blocks, uint32_t pc_step) {
    if ((!blocks && n_blocks) || n_blocks >= ((size_t)1 << 31)) return false;
    for (size_t b = 0; b < n_blocks; ++b) {
        const u64 end = (u64)blocks[b].start_pc + (u64)pc_step * blocks[b].n_instructions;
        if (!blocks[b].n_instructions || end > (b + 1 < n_blocks ? (u64)blocks[b + 1].start_pc : (u64)1 << 32)) return false;
    }
    return true;
}

// The buffers of the stage, part of the scratch of the context that declares it. icount: the 8 device counters, for a caller whose
// own kernels count in counters[3 ..] as well (counters()).
struct Stage : Scratch {
    explicit Stage(Scratch& owner) : Scratch(owner) {}
    Buf icount{*this}, tkey{*this}, tkey_s{*this}, idx{*this}, idx_s{*this}, pcs{*this}, pc_t{*this};
    u64* counters() { return icount.as<u64>(); }
};
// the names the stage's launches are timed under (the tools read them)
struct Names { const char *index, *sort, *time; };

// The M rows of `parts` by time key: s.tkey_s / s.idx_s hold the sorted keys and row numbers, s.pc_t the pcs in time order, counters[8]
// the device counters read back. g0[k] = the global number of part k's first row (trace_entry.hpp's Bridge numbers them through).
// d_counters: where the caller keeps its 8 counters, NULL = in the stage's own icount; they start as {0, kEmpty, kEmpty, ...} here.
// temp: the caller's temporary storage, which its later stages reuse. *status = 7 or 4 with *info where the rows are no execution;
// then nothing else is valid.
inline int rows_in_time_order(const PwSegmentAir* airs, const uint32_t* segment_of_air, const std::vector<Part>& parts, const std::vector<u64>& g0, u64 M,
                              Stage& s, u64* d_counters, Scratch::Buf& temp, Names names, u64* counters, uint32_t* status, uint64_t* info) {
    hipStream_t st = stream();
    if (!d_counters) {
        PW_TRY(s.icount.ensure(64));
        d_counters = s.counters();
    }
    static const u64 counters0[8] = {0, kEmpty, kEmpty, kEmpty, kEmpty, 0, 0, 0};
    PW_HIP_TRY(hipMemcpyAsync(d_counters, counters0, sizeof counters0, hipMemcpyHostToDevice, st));
    PW_TRY(s.tkey.ensure(M * 8));
    PW_TRY(s.tkey_s.ensure(M * 8));
    PW_TRY(s.idx.ensure(M * 4));
    PW_TRY(s.idx_s.ensure(M * 4));
    PW_TRY(s.pcs.ensure(M * 4));
    PW_TRY(s.pc_t.ensure(M * 4));
    {
        ScopedKernelTimer timer(names.index);
        for (size_t k = 0; k < parts.size(); ++k) {
            const Part& part = parts[k];
            const Walked w = walked(airs[part.air]);
            const uint32_t seg = segment_of_air ? segment_of_air[part.air] : 0u;
            with_fast(w.lp, [&](auto fast) {
                hipLaunchKernelGGL(empirical_index_kernel<decltype(fast)::value>, dim3(div_up(w.H, kBlock)), dim3(kBlock), 0, st, part.vals, w.H, w.lp, w.order, part.begin,
                                   part.end, (uint32_t)part.air, seg, g0[k], s.tkey.as<u64>(), s.pcs.as<uint32_t>(), d_counters);
            });
        }
        hipLaunchKernelGGL(empirical_iota_kernel, dim3(div_up(M, kBlock)), dim3(kBlock), 0, st, s.idx.as<uint32_t>(), M);
    }
    PW_HIP_TRY(hipGetLastError());
    {
        ScopedKernelTimer timer(names.sort);
        PW_TRY(with_temp(temp, [&](void* t, size_t& b) {
            return rocprim::radix_sort_pairs(t, b, s.tkey.as<u64>(), s.tkey_s.as<u64>(), s.idx.as<uint32_t>(), s.idx_s.as<uint32_t>(), (size_t)M, 0u, 64u, st);
        }));
    }
    {
        ScopedKernelTimer timer(names.time);
        hipLaunchKernelGGL(empirical_time_kernel, dim3(div_up(M, kBlock)), dim3(kBlock), 0, st, (const u64*)s.tkey_s.p, (const uint32_t*)s.idx_s.p,
                           (const uint32_t*)s.pcs.p, M, s.pc_t.as<uint32_t>(), d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, 8 * sizeof(u64), hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    if (counters[1] != kEmpty) {
        *status = 7;
        *info = counters[1];
    } else if (counters[2] != kEmpty) {
        *status = 4;
        *info = counters[2];
    }
    return 0;
}

}  // namespace time_index
}  // namespace pw
