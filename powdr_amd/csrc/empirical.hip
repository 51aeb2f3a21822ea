// Empirical constraints on the device (include/powdr_prover.h pw_empirical_detect): per executed pc the 1st and 99th
// percentile of every main column, per listed basic block the partition of its cells into classes that held equal values in every
// instance of the block — from the instruction AIRs' raw traces, read through the provers' own execution-bridge interactions.
//   index      time_index.hpp             the executed rows by time key and their pcs in time order (statuses 7 and 4): the stage shared
//                                         with the superblock detector (execution_blocks.hip, §5q)
//   structure  empirical_structure_kernel every row looks its pc up in the block table: a head checks the pcs of the rows behind it,
//                                         any other in-block row that its head is where it must be (status 3)
//   runs       a STABLE radix sort by pc keeps the time order inside a pc: one contiguous run per pc whose j-th row belongs to the
//              j-th instance of the pc's block; run-length encoding gives the pcs and their counts; empirical_loc_kernel turns row
//              numbers into (air, row) and finds a pc with rows of two AIRs (status 5)
//   panels     per panel of columns within the scratch bound: empirical_gather_kernel writes [column][position in the pc order] as
//              (column, run) << 32 | canonical value (coalesced writes); empirical_fingerprint_kernel adds H(seed, j, value) of every
//              cell of a run into the run's 128-bit sum — integer additions, kept in registers over 16 positions per lane and merged
//              per wave: one pair of global atomics per (wave, run, column), never per row; a radix sort of the panel sorts every (column, run) by canonical value and
//              empirical_pick_kernel reads the two percentile elements
//   classes    the host groups a block's cells by fingerprint (small), empirical_verify_kernel compares every member of a candidate
//              class with the class's first cell over all instances; a mismatch repeats the fingerprints under another seed
// No table here: of bus_shared.hpp this file takes the AIRs on the bridge bus (collect_parts), their launch (walked, with_fast) and
// the default scratch bound.
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

#include <memory>
#include <tuple>

struct PwEmpirical {
    std::vector<uint32_t> pcs, air_of_pc;
    std::vector<uint64_t> counts, range_off;   // range_off: n_pcs + 1
    std::vector<uint32_t> ranges;              // (lo, hi) pairs
    std::vector<uint32_t> blocks;              // the start pcs of the listed blocks that ran
    std::vector<uint64_t> class_off, cell_off; // n_blocks + 1 | n_classes + 1
    std::vector<uint32_t> cells;               // (instruction_idx, column_idx) pairs
};

namespace pw {

namespace {

using namespace bus;
using namespace time_index;

constexpr int kMergeRounds = 4;            // distinct runs a wave merges before its lanes fall back to one atomic each
constexpr uint32_t kVerifyChunk = 1024;    // instances a workgroup of the verification compares
constexpr int kSeeds = 3;                  // groupings tried before status 6
constexpr int kFpItems = 16;               // positions a lane of the fingerprint kernel walks before its wave merges

struct EAir { const uint32_t* trace; u64 H; uint32_t width, pad; };
struct EPart { u64 g0; uint32_t air, pad; };
struct VPair { uint32_t ra, ca, rf, cf; };

__host__ __device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A head (instruction 0 of a listed block) checks the pcs of the n - 1 rows behind it; any other in-block row checks that the row k
// places before it is its block's head. The smallest key among the offenders is what a sequential walk in time order meets first.
__global__ __launch_bounds__(kBlock) void empirical_structure_kernel(const u64* __restrict__ tkey_s, const uint32_t* __restrict__ pc_t, u64 N,
                                                                      const PwBasicBlock* __restrict__ blocks, uint32_t n_blocks, uint32_t pc_step,
                                                                      u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    uint32_t b, k;
    if (!find_block(blocks, n_blocks, pc_step, pc_t[i], &b, &k)) return;
    const PwBasicBlock B = blocks[b];
    bool ok = true;
    if (k == 0u) {
        for (uint32_t j = 1; ok && j < B.n_instructions; ++j) ok = i + j < N && pc_t[i + j] == B.start_pc + j * pc_step;
    } else {
        ok = i >= k && pc_t[i - k] == B.start_pc;
    }
    if (!ok) atomicMin(counters + 3, tkey_s[i]);
}

__device__ __forceinline__ u64 loc_of(const EPart* __restrict__ parts, uint32_t n_parts, u64 g) {
    uint32_t lo = 0, hi = n_parts;  // the last part with g0 <= g
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (parts[mid].g0 <= g) lo = mid + 1;
        else hi = mid;
    }
    const EPart p = parts[lo - 1];
    return ((u64)p.air << 32) | (g - p.g0);
}

// over the rows in (pc, time) order: (air << 32 | row) of every row, and a pc whose neighbouring rows lie in two AIRs
__global__ __launch_bounds__(kBlock) void empirical_loc_kernel(const uint32_t* __restrict__ pc_p, const uint32_t* __restrict__ idx_p, u64 N,
                                                                const EPart* __restrict__ parts, uint32_t n_parts, u64* __restrict__ loc_p,
                                                                u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const u64 loc = loc_of(parts, n_parts, idx_p[i]);
    loc_p[i] = loc;
    if (i && pc_p[i - 1] == pc_p[i] && (loc_of(parts, n_parts, idx_p[i - 1]) >> 32) != (loc >> 32)) atomicMin(counters + 4, (u64)pc_p[i]);
}

// run_of[i] = the run (pc) position i lies in; run_air[r] = the AIR of run r's first row
__global__ __launch_bounds__(kBlock) void empirical_runs_kernel(const uint32_t* __restrict__ start, uint32_t n_runs, const u64* __restrict__ loc_p, u64 N,
                                                                 uint32_t* __restrict__ run_of, uint32_t* __restrict__ run_air) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_runs) run_air[i] = (uint32_t)(loc_p[start[i]] >> 32);
    if (i >= N) return;
    uint32_t lo = 0, hi = n_runs;  // the last run with start <= i
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((u64)start[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    run_of[i] = lo - 1;
}

// keys[cc * N + i] = (cc * n_runs + run) << 32 | the canonical value of column c0 + cc at position i (0 where the row's AIR has no
// such column: the slot is sorted with its run and never read). blockIdx.y = cc: a wave writes 512 contiguous bytes.
__global__ __launch_bounds__(kBlock) void empirical_gather_kernel(const u64* __restrict__ loc_p, const uint32_t* __restrict__ run_of, u64 N, const EAir* __restrict__ airs,
                                                                   uint32_t c0, uint32_t n_runs, u64* __restrict__ keys) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const uint32_t cc = blockIdx.y, c = c0 + cc;
    const u64 loc = loc_p[i];
    const EAir a = airs[loc >> 32];
    const uint32_t v = c < a.width ? bb::from_monty(a.trace[(size_t)c * a.H + (size_t)(loc & 0xffffffffull)]) : 0u;
    keys[(u64)cc * N + i] = ((u64)(cc * n_runs + run_of[i]) << 32) | (u64)v;
}

// the lanes of a wave add what they hold into fps[2 * (range_off[run] + c)]: the runs are contiguous, so a wave holds a handful of
// them and each costs it ONE pair of atomics (wave-uniform: every lane calls it, a lane with run == kNoPc holds nothing)
__device__ __forceinline__ void fingerprint_merge(uint32_t run, u64 h0, u64 h1, uint32_t c, const u64* __restrict__ range_off, u64* __restrict__ fps) {
    const unsigned lane = threadIdx.x & 63u;
    u64 todo = __builtin_amdgcn_ballot_w64(run != kNoPc);
    for (int round = 0; round < kMergeRounds && todo; ++round) {
        const int leader = __builtin_ctzll(todo);
        const uint32_t key = (uint32_t)__shfl((int)run, leader, 64);
        const bool mine = run == key;
        const u64 s0 = wave_sum(mine ? h0 : 0ull), s1 = wave_sum(mine ? h1 : 0ull);
        if (lane == (unsigned)leader) {
            u64* at = fps + 2 * (range_off[key] + c);
            atomicAdd(at, s0);
            atomicAdd(at + 1, s1);
        }
        todo &= ~__builtin_amdgcn_ballot_w64(mine);
    }
    if ((todo >> lane) & 1ull) {  // (a wave over many short runs: every lane its own run, no hot address)
        u64* at = fps + 2 * (range_off[run] + c);
        atomicAdd(at, h0);
        atomicAdd(at + 1, h1);
    }
}

// fps[2 * (range_off[run] + c)] += H(seed, j, value), j = the position inside the run = the instance. A lane walks kFpItems
// positions a workgroup apart (coalesced) and keeps its sums in registers while they stay in one run; when any lane of the wave
// moves on to another run the whole wave merges what it holds (the branch is wave-uniform). On a hot pc a wave issues one pair of
// atomics per kFpItems x 64 rows.
__global__ __launch_bounds__(kBlock) void empirical_fingerprint_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ run_of, const uint32_t* __restrict__ start,
                                                                        const uint32_t* __restrict__ run_air, const u64* __restrict__ range_off, u64 N,
                                                                        const EAir* __restrict__ airs, uint32_t c0, u64 seed0, u64 seed1, u64* __restrict__ fps) {
    const u64 first = (u64)blockIdx.x * kBlock * kFpItems + threadIdx.x;
    const uint32_t cc = blockIdx.y, c = c0 + cc;
    uint32_t cur = kNoPc;
    u64 a0 = 0, a1 = 0;
    for (int it = 0; it < kFpItems; ++it) {
        const u64 i = first + (u64)it * kBlock;
        uint32_t run = kNoPc;
        u64 h0 = 0, h1 = 0;
        if (i < N) {
            const uint32_t r = run_of[i];
            if (c < airs[run_air[r]].width) {
                run = r;
                const u64 v = keys[(u64)cc * N + i] & 0xffffffffull, j = i - start[r];
                h0 = mix64(seed0 + ((j << 32) | v) * 0x9E3779B97F4A7C15ull);
                h1 = mix64(seed1 ^ ((v << 32) | j));
            }
        }
        if (__builtin_amdgcn_ballot_w64(cur != kNoPc && run != kNoPc && run != cur)) {
            fingerprint_merge(cur, a0, a1, c, range_off, fps);
            cur = kNoPc;
            a0 = a1 = 0;
        }
        if (run != kNoPc) {
            cur = run;
            a0 += h0;
            a1 += h1;
        }
    }
    fingerprint_merge(cur, a0, a1, c, range_off, fps);
}

// ranges[2 * (range_off[r] + c)] = the elements n / 100 and n * 99 / 100 of run r's sorted column c
__global__ __launch_bounds__(kBlock) void empirical_pick_kernel(const u64* __restrict__ sorted, const uint32_t* __restrict__ start, const uint32_t* __restrict__ count,
                                                                 const uint32_t* __restrict__ run_air, const u64* __restrict__ range_off, uint32_t n_runs, u64 N,
                                                                 const EAir* __restrict__ airs, uint32_t c0, uint32_t* __restrict__ ranges) {
    const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
    if (r >= n_runs) return;
    const uint32_t cc = blockIdx.y, c = c0 + cc;
    if (c >= airs[run_air[r]].width) return;
    const u64 n = count[r], base = (u64)cc * N + start[r];
    uint32_t* out = ranges + 2 * (range_off[r] + c);
    out[0] = (uint32_t)sorted[base + n / 100];
    out[1] = (uint32_t)sorted[base + n * 99 / 100];
}

// item = (pair, chunk): cell (ra, ca) against its class's first cell (rf, cf) over the chunk's instances
__global__ __launch_bounds__(kBlock) void empirical_verify_kernel(const VPair* __restrict__ pairs, const uint32_t* __restrict__ items, const uint32_t* __restrict__ start,
                                                                   const uint32_t* __restrict__ count, const u64* __restrict__ loc_p, const EAir* __restrict__ airs,
                                                                   uint32_t* __restrict__ mismatch) {
    const uint32_t p = items[2 * (size_t)blockIdx.x], chunk = items[2 * (size_t)blockIdx.x + 1];
    const VPair v = pairs[p];
    const u64 n = count[v.ra], sa = start[v.ra], sf = start[v.rf];
    const u64 last = ((u64)chunk + 1) * kVerifyChunk, end = n < last ? n : last;
    bool differ = false;
    for (u64 j = (u64)chunk * kVerifyChunk + threadIdx.x; j < end; j += kBlock) {
        const u64 la = loc_p[sa + j], lf = loc_p[sf + j];
        const EAir A = airs[la >> 32], F = airs[lf >> 32];
        const uint32_t a = A.trace[(size_t)v.ca * A.H + (size_t)(la & 0xffffffffull)], f = F.trace[(size_t)v.cf * F.H + (size_t)(lf & 0xffffffffull)];
        differ |= bb::from_monty(a) != bb::from_monty(f);
    }
    if (differ) mismatch[p] = 1u;
}

struct EmpCtx : Scratch {
    Buf small{*this, kStays};  // the index stage's counters (the kernels here count in them too) | AIR table | part table | block table
    time_index::Stage index{*this};
    Buf pc_p{*this}, idx_p{*this}, loc{*this}, uniq{*this}, cnt{*this}, start{*this}, run_of{*this}, run_air{*this}, range_off{*this}, ranges{*this}, fps{*this},
        keys{*this}, sorted{*this}, temp{*this}, pairs{*this}, items{*this}, mismatch{*this};
    uint64_t mask = 0;  // 0: the full width
    uint64_t stat_panels = 0, stat_seeds = 0, stat_rows = 0, stat_verified = 0;
    void reset_stats() override { stat_panels = stat_seeds = stat_rows = stat_verified = 0; }
};
thread_local EmpCtx g_emp;

size_t sort_keys_temp(size_t n, unsigned end_bit) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (u64*)nullptr, (u64*)nullptr, n, 0u, end_bit, stream());
    return std::max<size_t>(bytes, 16);
}
unsigned key_bits(u64 segments) {
    unsigned b = 1;
    while (b < 32 && ((u64)1 << b) < segments) ++b;
    return 32 + b;
}

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" void pw_empirical_percentile_indices(uint64_t n, uint64_t* lo, uint64_t* hi) {
    if (lo) *lo = n / 100;
    if (hi) *hi = (uint64_t)((unsigned __int128)n * 99 / 100);
}

extern "C" void pw_empirical_set_fingerprint_mask(uint64_t mask) { g_emp.mask = mask; }

extern "C" void pw_empirical_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_emp.stat_panels;
    out[1] = g_emp.stat_seeds;
    out[2] = g_emp.stat_rows;
    out[3] = g_emp.stat_verified;
    out[4] = g_emp.peak();
    out[5] = g_emp.held();
}

extern "C" void pw_empirical_destroy(PwEmpirical* e) { delete e; }

extern "C" void pw_empirical_sizes(const PwEmpirical* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->pcs.size();
    sizes[1] = e->ranges.size() / 2;
    sizes[2] = e->blocks.size();
    sizes[3] = e->cell_off.size() - 1;
    sizes[4] = e->cells.size() / 2;
}

extern "C" void pw_empirical_read_pcs(const PwEmpirical* e, uint32_t* pcs, uint64_t* counts, uint32_t* air_of_pc, uint64_t* range_offsets) {
    if (!e) return;
    if (pcs) std::copy(e->pcs.begin(), e->pcs.end(), pcs);
    if (counts) std::copy(e->counts.begin(), e->counts.end(), counts);
    if (air_of_pc) std::copy(e->air_of_pc.begin(), e->air_of_pc.end(), air_of_pc);
    if (range_offsets) std::copy(e->range_off.begin(), e->range_off.end(), range_offsets);
}

extern "C" void pw_empirical_read_ranges(const PwEmpirical* e, uint32_t* lo_hi) {
    if (e && lo_hi) std::copy(e->ranges.begin(), e->ranges.end(), lo_hi);
}

extern "C" void pw_empirical_read_blocks(const PwEmpirical* e, uint32_t* start_pcs, uint64_t* class_offsets, uint64_t* cell_offsets) {
    if (!e) return;
    if (start_pcs) std::copy(e->blocks.begin(), e->blocks.end(), start_pcs);
    if (class_offsets) std::copy(e->class_off.begin(), e->class_off.end(), class_offsets);
    if (cell_offsets) std::copy(e->cell_off.begin(), e->cell_off.end(), cell_offsets);
}

extern "C" void pw_empirical_read_cells(const PwEmpirical* e, uint32_t* instruction_column) {
    if (e && instruction_column) std::copy(e->cells.begin(), e->cells.end(), instruction_column);
}

extern "C" int pw_empirical_detect(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, uint32_t pc_step, const PwBasicBlock* blocks,
                                   size_t n_blocks, size_t scratch_bytes, PwEmpirical** out, uint32_t* status, uint64_t* info) {
    if (!out || !status || !info || !pc_step || bus >= bb::P || !airs_well_formed(airs, n_airs)) return -1;
    if (!blocks_well_formed(blocks, n_blocks, pc_step)) return -1;
    Bridge B;
    if (!bridge_of(airs, n_airs, bus, &B) || B.M >= ((u64)1 << 32)) return -1;  // row numbers and run positions are 32-bit words
    const u64 M = B.M;
    EmpCtx& cx = g_emp;
    const ScratchCall call(cx, out, status, info);
    auto result = std::make_unique<PwEmpirical>();
    result->range_off.push_back(0);
    result->class_off.push_back(0);
    result->cell_off.push_back(0);
    if (!M) {
        *out = result.release();
        return 0;
    }
    hipStream_t st = stream();

    std::vector<EPart> h_parts;
    std::vector<EAir> h_airs(n_airs, EAir{nullptr, 0, 0, 0});
    for (size_t a = 0; a < n_airs; ++a) h_airs[a] = EAir{airs[a].d_trace, (u64)1 << airs[a].log_height, airs[a].prover->width, 0};
    uint32_t max_width = 0;
    for (size_t k = 0; k < B.n_parts(); ++k) {
        h_parts.push_back(EPart{B.g0[k], (uint32_t)B.part_air[k], 0});
        max_width = std::max(max_width, airs[B.part_air[k]].prover->width);
    }

    // small: counters (8 u64) | AIR table | part table | block table
    const size_t off_air = 64, off_part = off_air + n_airs * sizeof(EAir), off_blocks = off_part + h_parts.size() * sizeof(EPart),
                 small_bytes = off_blocks + std::max<size_t>(n_blocks, 1) * sizeof(PwBasicBlock);
    PW_TRY(cx.small.ensure(small_bytes));
    char* base = cx.small.as<char>();
    u64* d_counters = (u64*)base;
    const EAir* d_airs = (const EAir*)(base + off_air);
    const EPart* d_parts = (const EPart*)(base + off_part);
    const PwBasicBlock* d_blocks = (const PwBasicBlock*)(base + off_blocks);

    // the bound: the caller's, or half of what the device has room for
    const size_t bound = call.bound(scratch_bytes);
    // the index stage holds 32 bytes per row and a sort's temporary storage; one column of a panel 16 bytes per active row (at most M)
    const size_t index_need = small_bytes - 64 + bytes_needed(M);  // (its 64 bytes of counters lie in `small`)
    auto panel_need = [&](u64 N, uint32_t C, u64 n_runs, u64 n_cells) {
        // row locations, counts, runs | per run | ranges, fingerprints, the verification's pairs and items | the panel and its sort
        return small_bytes + (size_t)N * 16 + (size_t)n_runs * 16 + 64 + (size_t)n_cells * 56 + (size_t)N * max_width / 128 * 8 + (size_t)N * C * 16 +
               sort_keys_temp(N * C, key_bits(n_runs * C));
    };
    if (bound < index_need) {
        *status = 2;
        *info = std::max(index_need, panel_need(M, 1, 0, 0));  // (what is known before a row is read; a later status 2 is exact)
        return 0;
    }

    PW_HIP_TRY(hipMemcpyAsync((void*)d_airs, h_airs.data(), n_airs * sizeof(EAir), hipMemcpyHostToDevice, st));
    PW_HIP_TRY(hipMemcpyAsync((void*)d_parts, h_parts.data(), h_parts.size() * sizeof(EPart), hipMemcpyHostToDevice, st));
    if (n_blocks) PW_HIP_TRY(hipMemcpyAsync((void*)d_blocks, blocks, n_blocks * sizeof(PwBasicBlock), hipMemcpyHostToDevice, st));

    // ---- index (time_index.hpp) ----
    u64 counters[8], N = 0;
    PW_TRY(open(airs, segment_of_air, n_airs, bus, B, cx.index, cx.temp, Names{"empirical_index_kernel", "empirical_sort_time", "empirical_structure_kernel"}, &N, status, info,
                d_counters, counters));
    if (*status) return (int)hipGetLastError();
    cx.stat_rows = N;
    if (!N) {
        *out = result.release();
        return (int)hipGetLastError();
    }
    {
        ScopedKernelTimer timer("empirical_structure_kernel");
        hipLaunchKernelGGL(empirical_structure_kernel, dim3(div_up(N, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.index.tkey_s.p, (const uint32_t*)cx.index.pc_t.p, N, d_blocks,
                           (uint32_t)n_blocks, pc_step, d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    if (counters[3] != kEmpty) {
        *status = 3;
        *info = counters[3];
        return (int)hipGetLastError();
    }
    cx.index.release_except({&cx.index.pc_t, &cx.index.idx_s});

    // ---- runs ----
    PW_TRY(cx.pc_p.ensure(N * 4));
    PW_TRY(cx.idx_p.ensure(N * 4));
    PW_TRY(cx.loc.ensure(N * 8));
    PW_TRY(cx.uniq.ensure(N * 4));
    PW_TRY(cx.cnt.ensure(N * 4));
    {
        ScopedKernelTimer timer("empirical_sort_pc");
        size_t temp_bytes = 0, rle_bytes = 0;
        PW_HIP_TRY(rocprim::radix_sort_pairs(nullptr, temp_bytes, cx.index.pc_t.as<uint32_t>(), cx.pc_p.as<uint32_t>(), cx.index.idx_s.as<uint32_t>(), cx.idx_p.as<uint32_t>(),
                                             (size_t)N, 0u, 31u, st));
        PW_HIP_TRY(rocprim::run_length_encode(nullptr, rle_bytes, cx.pc_p.as<uint32_t>(), (unsigned int)N, cx.uniq.as<uint32_t>(), cx.cnt.as<uint32_t>(),
                                              (uint32_t*)(d_counters + 5), st));
        PW_TRY(cx.temp.ensure(std::max<size_t>(std::max(temp_bytes, rle_bytes), 16)));
        PW_HIP_TRY(rocprim::radix_sort_pairs(cx.temp.p, temp_bytes, cx.index.pc_t.as<uint32_t>(), cx.pc_p.as<uint32_t>(), cx.index.idx_s.as<uint32_t>(), cx.idx_p.as<uint32_t>(),
                                             (size_t)N, 0u, 31u, st));
        hipLaunchKernelGGL(empirical_loc_kernel, dim3(div_up(N, kBlock)), dim3(kBlock), 0, st, (const uint32_t*)cx.pc_p.p, (const uint32_t*)cx.idx_p.p, N, d_parts,
                           (uint32_t)h_parts.size(), cx.loc.as<u64>(), d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(rocprim::run_length_encode(cx.temp.p, rle_bytes, cx.pc_p.as<uint32_t>(), (unsigned int)N, cx.uniq.as<uint32_t>(), cx.cnt.as<uint32_t>(),
                                              (uint32_t*)(d_counters + 5), st));
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    if (counters[4] != kEmpty) {
        *status = 5;
        *info = counters[4];
        return (int)hipGetLastError();
    }
    cx.index.release();
    cx.idx_p.release();
    cx.pc_p.release();
    cx.temp.release();
    const uint32_t n_runs = (uint32_t)counters[5];
    std::vector<uint32_t> h_pc(n_runs), h_cnt(n_runs), h_start(n_runs), h_air(n_runs);
    PW_HIP_TRY(hipMemcpyAsync(h_pc.data(), cx.uniq.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipMemcpyAsync(h_cnt.data(), cx.cnt.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    {
        u64 s = 0;
        for (uint32_t r = 0; r < n_runs; ++r) {
            h_start[r] = (uint32_t)s;
            s += h_cnt[r];
        }
    }
    cx.uniq.release();
    PW_TRY(cx.start.ensure((size_t)n_runs * 4));
    PW_TRY(cx.run_air.ensure((size_t)n_runs * 4));
    PW_TRY(cx.run_of.ensure(N * 4));
    PW_TRY(cx.range_off.ensure(((size_t)n_runs + 1) * 8));
    PW_HIP_TRY(hipMemcpyAsync(cx.start.p, h_start.data(), (size_t)n_runs * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(empirical_runs_kernel, dim3(div_up(std::max<u64>(N, n_runs), kBlock)), dim3(kBlock), 0, st, (const uint32_t*)cx.start.p, n_runs,
                       (const u64*)cx.loc.p, N, cx.run_of.as<uint32_t>(), cx.run_air.as<uint32_t>());
    PW_HIP_TRY(hipGetLastError());
    PW_HIP_TRY(hipMemcpyAsync(h_air.data(), cx.run_air.p, (size_t)n_runs * 4, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    std::vector<u64> h_roff(n_runs + 1, 0);
    uint32_t widest = 0;
    for (uint32_t r = 0; r < n_runs; ++r) {
        const uint32_t w = h_airs[h_air[r]].width;
        h_roff[r + 1] = h_roff[r] + w;
        widest = std::max(widest, w);
    }
    const u64 n_cells = h_roff[n_runs];
    PW_HIP_TRY(hipMemcpyAsync(cx.range_off.p, h_roff.data(), h_roff.size() * 8, hipMemcpyHostToDevice, st));
    PW_TRY(cx.ranges.ensure(std::max<size_t>(n_cells * 8, 16)));
    PW_TRY(cx.fps.ensure(std::max<size_t>(n_cells * 16, 16)));

    // ---- panels ----
    uint32_t C = 0;
    if (widest) {
        C = widest;
        while (C && ((u64)C * N >= ((u64)1 << 32) || (u64)C * n_runs >= ((u64)1 << 31) || panel_need(N, C, n_runs, n_cells) > bound)) --C;
        if (!C) {
            *status = 2;
            *info = std::max(index_need, panel_need(N, 1, n_runs, n_cells));
            return (int)hipGetLastError();
        }
        PW_TRY(cx.keys.ensure((size_t)N * C * 8));
        PW_TRY(cx.sorted.ensure((size_t)N * C * 8));
        PW_TRY(cx.temp.ensure(sort_keys_temp(N * C, key_bits((u64)n_runs * C))));
    }
    auto run_panels = [&](bool with_ranges, u64 seed0, u64 seed1) -> int {
        PW_HIP_TRY(hipMemsetAsync(cx.fps.p, 0, std::max<size_t>(n_cells * 16, 16), st));
        for (uint32_t c0 = 0; c0 < widest; c0 += C) {
            const uint32_t cols = std::min(C, widest - c0);
            const dim3 grid(div_up(N, kBlock), cols);
            {
                ScopedKernelTimer timer("empirical_gather_kernel");
                hipLaunchKernelGGL(empirical_gather_kernel, grid, dim3(kBlock), 0, st, (const u64*)cx.loc.p, (const uint32_t*)cx.run_of.p, N, d_airs, c0, n_runs,
                                   cx.keys.as<u64>());
            }
            {
                ScopedKernelTimer timer("empirical_fingerprint_kernel");
                hipLaunchKernelGGL(empirical_fingerprint_kernel, dim3(div_up(N, (size_t)kBlock * kFpItems), cols), dim3(kBlock), 0, st, (const u64*)cx.keys.p, (const uint32_t*)cx.run_of.p, (const uint32_t*)cx.start.p,
                                   (const uint32_t*)cx.run_air.p, (const u64*)cx.range_off.p, N, d_airs, c0, seed0, seed1, cx.fps.as<u64>());
            }
            PW_HIP_TRY(hipGetLastError());
            if (!with_ranges) continue;
            ++cx.stat_panels;
            {
                ScopedKernelTimer timer("empirical_sort_cells");
                size_t temp_bytes = cx.temp.bytes;
                PW_HIP_TRY(rocprim::radix_sort_keys(cx.temp.p, temp_bytes, cx.keys.as<u64>(), cx.sorted.as<u64>(), (size_t)N * cols, 0u, key_bits((u64)n_runs * cols), st));
            }
            {
                ScopedKernelTimer timer("empirical_pick_kernel");
                hipLaunchKernelGGL(empirical_pick_kernel, dim3(div_up(n_runs, kBlock), cols), dim3(kBlock), 0, st, (const u64*)cx.sorted.p, (const uint32_t*)cx.start.p,
                                   (const uint32_t*)cx.cnt.p, (const uint32_t*)cx.run_air.p, (const u64*)cx.range_off.p, n_runs, N, d_airs, c0, cx.ranges.as<uint32_t>());
            }
            PW_HIP_TRY(hipGetLastError());
        }
        return 0;
    };

    // the listed blocks that ran, with the runs of their instructions
    struct Seen { uint32_t block; std::vector<uint32_t> runs; };
    std::vector<Seen> seen;
    for (size_t b = 0; b < n_blocks; ++b) {
        const auto head = std::lower_bound(h_pc.begin(), h_pc.end(), blocks[b].start_pc);
        if (head == h_pc.end() || *head != blocks[b].start_pc) continue;
        Seen s{(uint32_t)b, {}};
        for (uint32_t k = 0; k < blocks[b].n_instructions; ++k) {
            const auto at = std::lower_bound(h_pc.begin(), h_pc.end(), blocks[b].start_pc + k * pc_step);
            // (present with the head's count: the structure check)
            if (at == h_pc.end() || *at != blocks[b].start_pc + k * pc_step || h_cnt[at - h_pc.begin()] != h_cnt[head - h_pc.begin()]) return (int)hipErrorInvalidValue;
            s.runs.push_back((uint32_t)(at - h_pc.begin()));
        }
        seen.push_back(std::move(s));
    }

    std::vector<u64> h_fps(n_cells * 2);
    struct Cell { u64 f0, f1; uint32_t k, c; };
    std::vector<std::vector<std::vector<std::pair<uint32_t, uint32_t>>>> classes;  // per seen block: classes of (k, c)
    const u64 mask = cx.mask ? cx.mask : ~0ull;
    bool exact = false;
    for (int attempt = 0; attempt < kSeeds && !exact; ++attempt) {
        ++cx.stat_seeds;
        const u64 seed0 = mix64(0x656d7069726963ull + (u64)attempt), seed1 = mix64(0x636c6173736573ull + 31 * (u64)attempt);
        PW_TRY(run_panels(attempt == 0, seed0, seed1));
        if (n_cells) PW_HIP_TRY(hipMemcpyAsync(h_fps.data(), cx.fps.p, n_cells * 16, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        classes.assign(seen.size(), {});
        std::vector<VPair> pairs;
        std::vector<uint32_t> items;
        std::vector<Cell> cells;
        for (size_t s = 0; s < seen.size(); ++s) {
            cells.clear();
            for (uint32_t k = 0; k < seen[s].runs.size(); ++k) {
                const uint32_t r = seen[s].runs[k], w = h_airs[h_air[r]].width;
                for (uint32_t c = 0; c < w; ++c) cells.push_back(Cell{h_fps[2 * (h_roff[r] + c)] & mask, h_fps[2 * (h_roff[r] + c) + 1] & mask, k, c});
            }
            std::sort(cells.begin(), cells.end(), [](const Cell& x, const Cell& y) {
                return std::tie(x.f0, x.f1, x.k, x.c) < std::tie(y.f0, y.f1, y.k, y.c);
            });
            const u64 n_inst = h_cnt[seen[s].runs[0]];
            for (size_t i = 0; i < cells.size();) {
                size_t j = i + 1;
                while (j < cells.size() && cells[j].f0 == cells[i].f0 && cells[j].f1 == cells[i].f1) ++j;
                if (j - i >= 2) {
                    std::vector<std::pair<uint32_t, uint32_t>> cls;
                    for (size_t e = i; e < j; ++e) {
                        cls.emplace_back(cells[e].k, cells[e].c);
                        if (e == i) continue;
                        for (u64 ch = 0; ch * kVerifyChunk < n_inst; ++ch) {
                            items.push_back((uint32_t)pairs.size());
                            items.push_back((uint32_t)ch);
                        }
                        pairs.push_back(VPair{seen[s].runs[cells[e].k], cells[e].c, seen[s].runs[cells[i].k], cells[i].c});
                    }
                    classes[s].push_back(std::move(cls));
                }
                i = j;
            }
            std::sort(classes[s].begin(), classes[s].end());
        }
        exact = true;
        if (!pairs.empty()) {
            if (pairs.size() >= ((size_t)1 << 32) || items.size() / 2 >= ((size_t)1 << 31)) return (int)hipErrorInvalidValue;
            cx.stat_verified += pairs.size();
            PW_TRY(cx.pairs.ensure(pairs.size() * sizeof(VPair)));
            PW_TRY(cx.items.ensure(items.size() * 4));
            PW_TRY(cx.mismatch.ensure(pairs.size() * 4));
            PW_HIP_TRY(hipMemcpyAsync(cx.pairs.p, pairs.data(), pairs.size() * sizeof(VPair), hipMemcpyHostToDevice, st));
            PW_HIP_TRY(hipMemcpyAsync(cx.items.p, items.data(), items.size() * 4, hipMemcpyHostToDevice, st));
            PW_HIP_TRY(hipMemsetAsync(cx.mismatch.p, 0, pairs.size() * 4, st));
            {
                ScopedKernelTimer timer("empirical_verify_kernel");
                hipLaunchKernelGGL(empirical_verify_kernel, dim3((unsigned)(items.size() / 2)), dim3(kBlock), 0, st, (const VPair*)cx.pairs.p, (const uint32_t*)cx.items.p,
                                   (const uint32_t*)cx.start.p, (const uint32_t*)cx.cnt.p, (const u64*)cx.loc.p, d_airs, cx.mismatch.as<uint32_t>());
            }
            PW_HIP_TRY(hipGetLastError());
            std::vector<uint32_t> mism(pairs.size());
            PW_HIP_TRY(hipMemcpyAsync(mism.data(), cx.mismatch.p, pairs.size() * 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            exact = std::find(mism.begin(), mism.end(), 1u) == mism.end();
        }
    }
    if (!exact) {
        *status = 6;
        return (int)hipGetLastError();
    }

    // ---- the result, in canonical order ----
    PwEmpirical& R = *result;
    R.pcs = h_pc;
    R.air_of_pc = h_air;
    R.counts.assign(h_cnt.begin(), h_cnt.end());
    R.range_off.assign(h_roff.begin(), h_roff.end());
    R.ranges.resize(n_cells * 2);
    if (n_cells) PW_HIP_TRY(hipMemcpyAsync(R.ranges.data(), cx.ranges.p, n_cells * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    for (size_t s = 0; s < seen.size(); ++s) {
        R.blocks.push_back(blocks[seen[s].block].start_pc);
        for (const auto& cls : classes[s]) {
            for (const auto& cell : cls) {
                R.cells.push_back(cell.first);
                R.cells.push_back(cell.second);
            }
            R.cell_off.push_back(R.cells.size() / 2);
        }
        R.class_off.push_back(R.cell_off.size() - 1);
    }
    const int rc = (int)hipGetLastError();
    if (!rc) *out = result.release();
    return rc;
}
