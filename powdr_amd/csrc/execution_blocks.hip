// Superblock detection on the device (include/powdr_prover.h pw_execution_blocks_from_pcs): from the execution's pcs in
// order, the distinct runs of basic blocks with their counts, every window of up to max_bb blocks inside a run with its greedy
// non-overlapping count over all run instances, the count of every pc — and a resident copy of the head sequence on which candidates are
// re-counted and removed (the body of the reference's greedy selection loop).
//   heads      execution_blocks_heads_kernel   one lane per position looks its pc and its predecessor's up in the block table: the
//                                              position is consistent with a sequential walk iff it continues its predecessor's block
//                                              or starts a block right after a block's last instruction; the smallest inconsistent
//                                              position (a min-reduction) is what the walk meets first (status 3). Compactions give the
//                                              heads, then the multi-instruction heads S[0..K) with run start flags; scans give run ids
//   pcs        a radix sort of the pcs and a run-length encoding
//   runs       H(seed, j, block) of every element, summed per run by a segmented reduction (no atomics: a hot run is one segment);
//              a radix sort of the runs by a key of (length, fingerprint); every run is VERIFIED element by element against the first
//              run of its group, one lane per element; a mismatch repeats the fingerprints under another seed
//   levels     per window length L: key = (name of the window of length L - 1, last block), a stable radix sort of (key, position) —
//              which is also the order the counts need — flags and scans give the dense names of the next level; two occurrences of
//              a window conflict iff their positions differ by less than L: a maximal stretch of such neighbours is a cluster, its
//              first element is always taken; a cluster of one counts one (the common case), in a longer one every element takes
//              nxt = the first element at least L further on (a binary search over at most L neighbours) and the length of the chain
//              from the cluster's first element comes from pointer doubling (log2 of the longest cluster rounds); a segmented
//              reduction adds the clusters of a window. Nothing walks a group sequentially and no address is hit once per element.
//   count      the same greedy pass over the positions where the needle matches inside one run; removal keeps the doubling tables,
//              marks the chain from coarse to fine and overwrites the chosen windows with a block no needle has
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

#include <memory>

namespace pw {

namespace {

using namespace bus;
using time_index::find_block;

constexpr uint32_t kNone = 0xffffffffu;
constexpr int kSeeds = 3;  // groupings tried before status 6
constexpr u64 kLow = 0xffffffffull;

struct NotNone32 { __device__ bool operator()(uint32_t x) const { return x != kNone; } };
struct NotEmpty64 { __device__ bool operator()(u64 x) const { return x != kEmpty; } };

__host__ __device__ __forceinline__ u64 mix64(u64 z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// counters: [0] the smallest offending position (or its time key) | [1] a run that differs from its group's first | [2] the longest
// cluster | [3] clusters of more than one element
// head[i] = the block that starts at position i, kNone elsewhere. Position i is consistent iff its pc is instruction k > 0 of a block
// and pc[i - 1] is instruction k - 1, or it is instruction 0 and i == 0 or pc[i - 1] is the last instruction of its block.
__global__ __launch_bounds__(kBlock) void execution_blocks_heads_kernel(const uint32_t* __restrict__ pc, u64 N, const PwBasicBlock* __restrict__ blocks, uint32_t n_blocks,
                                                                         uint32_t pc_step, const u64* __restrict__ tkey, uint32_t* __restrict__ head,
                                                                         u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (i < N) {
        uint32_t b = 0, k = 0, pb = 0, pk = 0;
        const uint32_t me = pc[i];
        bool ok = find_block(blocks, n_blocks, pc_step, me, &b, &k);
        if (ok && k) ok = i && pc[i - 1] == me - pc_step;
        else if (ok && i) ok = find_block(blocks, n_blocks, pc_step, pc[i - 1], &pb, &pk) && pk + 1 == blocks[pb].n_instructions;
        head[i] = ok && !k ? b : kNone;
        bad = !ok;
    }
    if (__builtin_amdgcn_ballot_w64(bad)) {
        const u64 w = wave_min(bad ? (tkey ? tkey[i] : i) : kEmpty);
        if ((threadIdx.x & 63u) == 0u) atomicMin(counters, w);
    }
}

// over the heads: a multi-instruction head as (starts a run) << 32 | block, a one-instruction head as kEmpty
__global__ __launch_bounds__(kBlock) void execution_blocks_cut_kernel(const uint32_t* __restrict__ B, u64 M, const PwBasicBlock* __restrict__ blocks, u64* __restrict__ packed) {
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (j >= M) return;
    const uint32_t b = B[j];
    const bool start = !j || blocks[B[j - 1]].n_instructions == 1u;
    packed[j] = blocks[b].n_instructions == 1u ? kEmpty : ((u64)start << 32) | b;
}

__global__ __launch_bounds__(kBlock) void execution_blocks_unpack_kernel(const u64* __restrict__ packed, u64 K, uint32_t* __restrict__ S, uint32_t* __restrict__ sflag) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    S[i] = (uint32_t)packed[i];
    sflag[i] = (uint32_t)(packed[i] >> 32);
}

// rid[i] = the run of element i plus one, rs[r] = the first element of run r (rs[R] = K)
__global__ __launch_bounds__(kBlock) void execution_blocks_hash_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ rs, u64 K,
                                                                        u64 seed0, u64 seed1, u64* __restrict__ h0, u64* __restrict__ h1) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const u64 v = S[i], j = i - rs[rid[i] - 1u];
    h0[i] = mix64(seed0 + ((j << 32) | v) * 0x9E3779B97F4A7C15ull);
    h1[i] = mix64(seed1 ^ ((v << 32) | j));
}

__global__ __launch_bounds__(kBlock) void execution_blocks_runkey_kernel(const u64* __restrict__ fp0, const u64* __restrict__ fp1, const uint32_t* __restrict__ rs, u64 R,
                                                                          u64 mask, u64* __restrict__ key, uint32_t* __restrict__ idx) {
    const u64 r = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (r >= R) return;
    const u64 len = rs[r + 1] - rs[r];
    key[r] = mix64((fp0[r] & mask) ^ mix64((fp1[r] & mask) + len * 0x9E3779B97F4A7C15ull));
    idx[r] = (uint32_t)r;
}

// first[t] = t where a group of equal keys starts, 0 elsewhere: a running maximum gives every element its group's first
__global__ __launch_bounds__(kBlock) void execution_blocks_group_kernel(const u64* __restrict__ key_s, u64 R, uint32_t* __restrict__ first) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t < R) first[t] = t && key_s[t] != key_s[t - 1] ? (uint32_t)t : 0u;
}

__global__ __launch_bounds__(kBlock) void execution_blocks_first_kernel(const uint32_t* __restrict__ idx_s, const uint32_t* __restrict__ first, u64 R,
                                                                         uint32_t* __restrict__ first_run) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t < R) first_run[idx_s[t]] = idx_s[first[t]];
}

// one lane per element: its run against the first run of the run's group, length and element
__global__ __launch_bounds__(kBlock) void execution_blocks_verify_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ rs,
                                                                          const uint32_t* __restrict__ first_run, u64 K, u64* __restrict__ counters) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    const uint32_t r = rid[i] - 1u, f = first_run[r];
    if (f == r) return;
    const bool differ = rs[r + 1] - rs[r] != rs[f + 1] - rs[f] || S[rs[f] + (i - rs[r])] != S[i];
    if (differ) counters[1] = 1;  // (a plain store: every writer writes the same word)
}

// key of the window of length L at i: (name of its first L - 1 blocks) << bbits | its last block; `invalid` where it does not fit its run
__global__ __launch_bounds__(kBlock) void execution_blocks_key_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ rs,
                                                                       const uint32_t* __restrict__ id_prev, u64 K, uint32_t L, uint32_t bbits, u64 invalid,
                                                                       u64* __restrict__ key, uint32_t* __restrict__ pos) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    pos[i] = (uint32_t)i;
    if (i + L > (u64)rs[rid[i]]) key[i] = invalid;
    else key[i] = L == 1u ? (u64)S[i] : ((u64)id_prev[i] << bbits) | S[i + L - 1];
}

// over positions sorted by (key, position), group = key (key_s == nullptr: one group): hflag = a group starts; cval = t where a
// cluster starts (no neighbour of its group less than L before it), 0 elsewhere
__global__ __launch_bounds__(kBlock) void execution_blocks_flag_kernel(const u64* __restrict__ key_s, const uint32_t* __restrict__ pos_s, u64 n, uint32_t L,
                                                                        uint32_t* __restrict__ hflag, uint32_t* __restrict__ cval) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    const bool h = !t || (key_s && key_s[t] != key_s[t - 1]);
    const bool close = !h && pos_s[t] - pos_s[t - 1] < L;
    if (hflag) hflag[t] = h;
    cval[t] = close ? 0u : (uint32_t)t;
}

// id_next[position] = the dense name; val = 1 at a cluster's first element; counters[2] = the longest cluster (its last element knows)
__global__ __launch_bounds__(kBlock) void execution_blocks_level_kernel(const uint32_t* __restrict__ pos_s, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ cstart,
                                                                         u64 n, uint32_t* __restrict__ id_next, u64* __restrict__ val, u64* __restrict__ counters) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    u64 size = 0;
    if (t < n) {
        if (id_next) id_next[pos_s[t]] = rank[t] - 1u;
        val[t] = cstart[t] == t;
        size = t - cstart[t] + 1;
    }
    size = ~wave_min(~size);
    if ((threadIdx.x & 63u) == 0u && size > 1) atomicMax(counters + 2, size);
}

// state[t] = nxt << 32 | 1: nxt = the first element of t's cluster at least L positions further on, kNone if there is none. The
// candidates are the next L elements at most (positions grow by one or more), and "in my cluster and closer than L" holds for a
// prefix of them.
__global__ __launch_bounds__(kBlock) void execution_blocks_next_kernel(const uint32_t* __restrict__ pos_s, const uint32_t* __restrict__ cstart, u64 n, uint32_t L,
                                                                        u64* __restrict__ state, u64* __restrict__ counters) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    bool long_head = false;
    if (t < n) {
        const uint32_t c = cstart[t];
        const u64 want = (u64)pos_s[t] + L;
        u64 lo = t + 1, hi = t + 1 + L < n ? t + 1 + L : n;  // the first u in [lo, hi) that is not (in the cluster and before want)
        while (lo < hi) {
            const u64 mid = lo + (hi - lo) / 2;
            if (cstart[mid] == c && (u64)pos_s[mid] < want) lo = mid + 1;
            else hi = mid;
        }
        const bool found = lo < n && cstart[lo] == c;
        state[t] = ((found ? lo : (u64)kNone) << 32) | 1ull;
        long_head = c == t && t + 1 < n && cstart[t + 1] == c;
    }
    const u64 heads = __builtin_amdgcn_ballot_w64(long_head);
    if ((threadIdx.x & 63u) == 0u && heads) atomicAdd(counters + 3, (u64)__builtin_popcountll(heads));
}

// one round of pointer doubling: (jump, count) of t becomes (jump of jump, count + count of jump)
__global__ __launch_bounds__(kBlock) void execution_blocks_jump_kernel(const u64* __restrict__ from, u64* __restrict__ to, u64 n) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n) return;
    u64 s = from[t];
    if ((s >> 32) != kNone) {
        const u64 o = from[s >> 32];
        s = (o & ~kLow) | ((s & kLow) + (o & kLow));
    }
    to[t] = s;
}

__global__ __launch_bounds__(kBlock) void execution_blocks_chain_kernel(const u64* __restrict__ state, const uint32_t* __restrict__ cstart, u64 n, u64* __restrict__ val) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t < n && cstart[t] == t) val[t] = state[t] & kLow;
}

// ---- count / remove on the resident sequence ----
__global__ __launch_bounds__(kBlock) void execution_blocks_match_kernel(const uint32_t* __restrict__ S, const uint32_t* __restrict__ rid, u64 K, const uint32_t* __restrict__ needle,
                                                                         uint32_t L, uint32_t* __restrict__ flag) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= K) return;
    bool m = i + L <= K && rid[i + L - 1] == rid[i];
    for (uint32_t k = 0; m && k < L; ++k) m = S[i + k] == needle[k];
    flag[i] = m;
}

// chosen: every element a marked one jumps to by this table (the tables go from the longest jump to the shortest)
__global__ __launch_bounds__(kBlock) void execution_blocks_mark_kernel(const u64* __restrict__ table, u64 n, uint32_t* __restrict__ chosen) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n || !chosen[t]) return;
    const u64 j = table[t] >> 32;
    if (j != kNone) chosen[j] = 1u;
}

__global__ __launch_bounds__(kBlock) void execution_blocks_chosen_kernel(const uint32_t* __restrict__ cstart, u64 n, uint32_t* __restrict__ chosen) {
    const u64 t = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (t < n) chosen[t] = cstart[t] == t;
}

__global__ __launch_bounds__(kBlock) void execution_blocks_remove_kernel(const uint32_t* __restrict__ mp, const uint32_t* __restrict__ chosen, u64 n, uint32_t L,
                                                                          uint32_t* __restrict__ S) {
    const u64 x = (u64)blockIdx.x * kBlock + threadIdx.x;
    const u64 t = x / L;
    if (t < n && chosen[t]) S[(u64)mp[t] + x % L] = kNone;  // (inside [0, K): a match is a window that fits)
}

struct EbCtx : Scratch {
    Buf small{*this}, head{*this}, pc_s{*this}, uniq{*this}, cnt{*this}, B{*this}, packed{*this}, sflag{*this}, h0{*this}, h1{*this}, fp0{*this}, fp1{*this}, rkey{*this},
        rkey_s{*this}, ridx{*this}, ridx_s{*this}, first_run{*this}, id_a{*this}, id_b{*this}, key{*this}, key_s{*this}, pos{*this}, pos_s{*this}, hflag{*this}, rank{*this},
        cval{*this}, cstart{*this}, val{*this}, st_a{*this}, st_b{*this}, gkey{*this}, gsum{*this}, guniq{*this}, temp{*this}, rs{*this};
    time_index::Stage index{*this};  // of the trace route
    uint64_t mask = 0;  // 0: the full width
    uint64_t stat_levels = 0, stat_jumping = 0, stat_seeds = 0, stat_heads = 0, stat_runs = 0;
    void reset_stats() override { stat_levels = stat_jumping = stat_seeds = stat_heads = stat_runs = 0; }
};
thread_local EbCtx g_eb;

unsigned bits_for(u64 values) {  // bits that hold 0 .. values - 1
    unsigned b = 1;
    while (b < 63 && ((u64)1 << b) < values) ++b;
    return b;
}

// bytes per position of the heads stage and per element of the run and level stages (what the buffers above add up to), and the
// temporary storage of the largest sort
size_t heads_need(u64 N) { return 65536 + (size_t)N * 36; }
size_t levels_need(u64 K) { return 65536 + (size_t)K * 168; }

// The greedy non-overlapping count over n occurrences sorted by (group, position) — cval/cstart/val/st_a/st_b of cx are written; on
// return val[t] = the occurrences chosen in the cluster that starts at t, 0 elsewhere. tables (count's removal): every round of the
// doubling keeps its table, n words each, in *tables; *rounds says how many.
int greedy_chains(EbCtx& cx, const u64* key_s, const uint32_t* pos_s, u64 n, uint32_t L, uint32_t* hflag, uint32_t* rank, uint32_t* id_next, u64* d_counters,
                  DeviceBuf* tables, int* rounds) {
    hipStream_t st = stream();
    const dim3 grid(div_up(n, kBlock)), block(kBlock);
    PW_HIP_TRY(hipMemsetAsync(d_counters + 2, 0, 8, st));
    hipLaunchKernelGGL(execution_blocks_flag_kernel, grid, block, 0, st, key_s, pos_s, n, L, hflag, cx.cval.as<uint32_t>());
    if (hflag)
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, hflag, rank, (size_t)n, rocprim::plus<uint32_t>(), st); }));
    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
        return rocprim::inclusive_scan(t, b, cx.cval.as<uint32_t>(), cx.cstart.as<uint32_t>(), (size_t)n, rocprim::maximum<uint32_t>(), st);
    }));
    hipLaunchKernelGGL(execution_blocks_level_kernel, grid, block, 0, st, pos_s, (const uint32_t*)rank, (const uint32_t*)cx.cstart.p, n, id_next, cx.val.as<u64>(), d_counters);
    PW_HIP_TRY(hipGetLastError());
    u64 longest = 0;
    PW_HIP_TRY(hipMemcpyAsync(&longest, d_counters + 2, 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    if (rounds) *rounds = 0;
    if (longest <= 1) return 0;
    int r = 0;
    while (((u64)1 << r) < longest) ++r;
    u64 *from = cx.st_a.as<u64>(), *to = cx.st_b.as<u64>();
    if (tables) {
        PW_TRY(tables->ensure((size_t)(r + 1) * n * 8));
        from = tables->as<u64>();
    }
    hipLaunchKernelGGL(execution_blocks_next_kernel, grid, block, 0, st, pos_s, (const uint32_t*)cx.cstart.p, n, L, from, d_counters);
    for (int k = 0; k < r; ++k) {
        if (tables) to = from + n;
        hipLaunchKernelGGL(execution_blocks_jump_kernel, grid, block, 0, st, (const u64*)from, to, n);
        if (tables) from = to;
        else std::swap(from, to);
    }
    hipLaunchKernelGGL(execution_blocks_chain_kernel, grid, block, 0, st, (const u64*)from, (const uint32_t*)cx.cstart.p, n, cx.val.as<u64>());
    PW_HIP_TRY(hipGetLastError());
    if (rounds) *rounds = r;
    return 0;
}

}  // namespace

}  // namespace pw

using namespace pw;

struct PwExecutionBlocks {
    std::vector<uint32_t> pcs, run_pcs, sb_pcs;
    std::vector<uint64_t> pc_counts, run_off, run_counts, sb_off, sb_counts;
    std::vector<PwBasicBlock> blocks;
    DeviceBuf S, rid;  // the resident head sequence: block indices (kNone = removed) and run ids
    u64 K = 0;
};

extern "C" void pw_execution_blocks_set_fingerprint_mask(uint64_t mask) { g_eb.mask = mask; }

extern "C" void pw_execution_blocks_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_eb.stat_levels;
    out[1] = g_eb.stat_jumping;
    out[2] = g_eb.stat_seeds;
    out[3] = g_eb.stat_heads;
    out[4] = g_eb.stat_runs;
    out[5] = g_eb.peak();
    out[6] = g_eb.held();
}

extern "C" void pw_execution_blocks_destroy(PwExecutionBlocks* e) { delete e; }

extern "C" void pw_execution_blocks_sizes(const PwExecutionBlocks* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->pcs.size();
    sizes[1] = e->run_counts.size();
    sizes[2] = e->run_pcs.size();
    sizes[3] = e->sb_counts.size();
    sizes[4] = e->sb_pcs.size();
    sizes[5] = e->K;
}

extern "C" void pw_execution_blocks_read_pc_counts(const PwExecutionBlocks* e, uint32_t* pcs, uint64_t* counts) {
    if (!e) return;
    if (pcs) std::copy(e->pcs.begin(), e->pcs.end(), pcs);
    if (counts) std::copy(e->pc_counts.begin(), e->pc_counts.end(), counts);
}

extern "C" void pw_execution_blocks_read_runs(const PwExecutionBlocks* e, uint64_t* offsets, uint32_t* start_pcs, uint64_t* counts) {
    if (!e) return;
    if (offsets) std::copy(e->run_off.begin(), e->run_off.end(), offsets);
    if (start_pcs) std::copy(e->run_pcs.begin(), e->run_pcs.end(), start_pcs);
    if (counts) std::copy(e->run_counts.begin(), e->run_counts.end(), counts);
}

extern "C" void pw_execution_blocks_read_superblocks(const PwExecutionBlocks* e, uint64_t* offsets, uint32_t* start_pcs, uint64_t* counts) {
    if (!e) return;
    if (offsets) std::copy(e->sb_off.begin(), e->sb_off.end(), offsets);
    if (start_pcs) std::copy(e->sb_pcs.begin(), e->sb_pcs.end(), start_pcs);
    if (counts) std::copy(e->sb_counts.begin(), e->sb_counts.end(), counts);
}

namespace {

std::unique_ptr<PwExecutionBlocks> empty_result(const PwBasicBlock* blocks, size_t n_blocks) {
    auto result = std::make_unique<PwExecutionBlocks>();
    result->run_off.push_back(0);
    result->sb_off.push_back(0);
    result->blocks.assign(blocks, blocks + n_blocks);
    return result;
}

// Everything behind the pcs in execution order: d_pcs[0..N), N > 0; d_tkey = their time keys where they come from traces (what status
// 3 names), nullptr = positions. `extra` = scratch bytes the caller holds through the heads stage. The caller releases cx's buffers.
int detect_blocks(EbCtx& cx, const uint32_t* d_pcs, const u64* d_tkey, u64 N, uint32_t pc_step, const PwBasicBlock* blocks, size_t n_blocks, uint32_t max_bb, size_t bound,
                  size_t extra, std::unique_ptr<PwExecutionBlocks>& result, uint32_t* status, uint64_t* info) {
    PwExecutionBlocks& R = *result;
    hipStream_t st = stream();
    if (bound < heads_need(N) + extra) {
        *status = 2;
        *info = std::max(heads_need(N) + extra, levels_need(N));  // (as many elements as positions at most)
        return 0;
    }

    // small: counters (8 u64) | block table
    const size_t off_blocks = 64, small_bytes = off_blocks + std::max<size_t>(n_blocks, 1) * sizeof(PwBasicBlock);
    PW_TRY(cx.small.ensure(small_bytes));
    u64* d_counters = cx.small.as<u64>();
    const PwBasicBlock* d_blocks = (const PwBasicBlock*)(cx.small.as<char>() + off_blocks);
    const u64 counters0[8] = {kEmpty, 0, 0, 0, 0, 0, 0, 0};
    PW_HIP_TRY(hipMemcpyAsync(d_counters, counters0, sizeof counters0, hipMemcpyHostToDevice, st));
    if (n_blocks) PW_HIP_TRY(hipMemcpyAsync((void*)d_blocks, blocks, n_blocks * sizeof(PwBasicBlock), hipMemcpyHostToDevice, st));
    uint32_t* d_n = (uint32_t*)(d_counters + 4);  // counts written by the compactions (counters[4..7])
    u64 counters[8];

    // ---- heads ----
    PW_TRY(cx.head.ensure(N * 4));
    PW_TRY(cx.B.ensure(N * 4));
    {
        ScopedKernelTimer timer("execution_blocks_heads_kernel");
        hipLaunchKernelGGL(execution_blocks_heads_kernel, dim3(div_up(N, kBlock)), dim3(kBlock), 0, st, d_pcs, N, d_blocks, (uint32_t)n_blocks, pc_step, d_tkey,
                           cx.head.as<uint32_t>(), d_counters);
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::select(t, b, cx.head.as<uint32_t>(), cx.B.as<uint32_t>(), d_n, (size_t)N, NotNone32(), st); }));
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    if (counters[0] != kEmpty) {
        *status = 3;
        *info = counters[0];
        return (int)hipGetLastError();
    }
    const u64 M = (uint32_t)counters[4];
    cx.stat_heads = M;
    cx.head.release();

    // ---- the pcs and their counts ----
    {
        ScopedKernelTimer timer("execution_blocks_pc_counts");
        PW_TRY(cx.pc_s.ensure(N * 4));
        PW_TRY(cx.uniq.ensure(N * 4));
        PW_TRY(cx.cnt.ensure(N * 4));
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, d_pcs, cx.pc_s.as<uint32_t>(), (size_t)N, 0u, 32u, st); }));
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::run_length_encode(t, b, cx.pc_s.as<uint32_t>(), (unsigned int)N, cx.uniq.as<uint32_t>(), cx.cnt.as<uint32_t>(), d_n + 1, st);
        }));
        uint32_t n_pcs = 0;
        PW_HIP_TRY(hipMemcpyAsync(&n_pcs, d_n + 1, 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        std::vector<uint32_t> h_cnt(n_pcs);
        R.pcs.resize(n_pcs);
        PW_HIP_TRY(hipMemcpyAsync(R.pcs.data(), cx.uniq.p, (size_t)n_pcs * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(h_cnt.data(), cx.cnt.p, (size_t)n_pcs * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        R.pc_counts.assign(h_cnt.begin(), h_cnt.end());
        cx.pc_s.release();
        cx.uniq.release();
        cx.cnt.release();
    }

    // ---- the multi-instruction heads S[0..K), their runs ----
    PW_TRY(cx.packed.ensure(M * 8));
    PW_TRY(cx.key.ensure(M * 8));  // (the compacted pairs; the levels' keys later)
    u64 K = 0, n_runs = 0;
    {
        ScopedKernelTimer timer("execution_blocks_cut_kernel");
        hipLaunchKernelGGL(execution_blocks_cut_kernel, dim3(div_up(M, kBlock)), dim3(kBlock), 0, st, (const uint32_t*)cx.B.p, M, d_blocks, cx.packed.as<u64>());
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::select(t, b, cx.packed.as<u64>(), cx.key.as<u64>(), d_n, (size_t)M, NotEmpty64(), st); }));
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        K = (uint32_t)counters[4];
    }
    cx.B.release();
    cx.packed.release();
    if (K && bound < levels_need(K)) {
        *status = 2;
        *info = std::max(heads_need(N) + extra, levels_need(K));
        return (int)hipGetLastError();
    }
    std::vector<uint32_t> h_S(K), h_rs;
    if (K) {
        ScopedKernelTimer timer("execution_blocks_runs");
        PW_TRY(R.S.ensure(K * 4));
        PW_TRY(R.rid.ensure(K * 4));
        PW_TRY(cx.sflag.ensure(K * 4));
        PW_TRY(cx.rs.ensure((K + 1) * 4));  // the run starts, rs[R] = K: kept through the levels
        cx.set_extra(R.S.bytes + R.rid.bytes);  // (the handle's part of the scratch from here on)
        hipLaunchKernelGGL(execution_blocks_unpack_kernel, dim3(div_up(K, kBlock)), dim3(kBlock), 0, st, (const u64*)cx.key.p, K, R.S.as<uint32_t>(), cx.sflag.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::inclusive_scan(t, b, cx.sflag.as<uint32_t>(), R.rid.as<uint32_t>(), (size_t)K, rocprim::plus<uint32_t>(), st);
        }));
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::select(t, b, rocprim::counting_iterator<uint32_t>(0), cx.sflag.as<uint32_t>(), cx.rs.as<uint32_t>(), d_n, (size_t)K, st);
        }));
        PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        n_runs = (uint32_t)counters[4];
        h_rs.resize(n_runs + 1);
        h_rs[n_runs] = (uint32_t)K;
        PW_HIP_TRY(hipMemcpyAsync(cx.rs.as<uint32_t>() + n_runs, &h_rs[n_runs], 4, hipMemcpyHostToDevice, st));
        PW_HIP_TRY(hipMemcpyAsync(h_rs.data(), cx.rs.p, n_runs * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(h_S.data(), R.S.p, K * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    cx.key.release();
    cx.stat_runs = n_runs;
    R.K = K;
    const uint32_t *d_S = R.S.as<uint32_t>(), *d_rid = R.rid.as<uint32_t>();

    // ---- distinct runs ----
    if (K) {
        const u64 Rn = n_runs;
        Scratch::Buf& rs = cx.rs;
        PW_TRY(cx.h0.ensure(K * 8));
        PW_TRY(cx.h1.ensure(K * 8));
        PW_TRY(cx.fp0.ensure(Rn * 8));
        PW_TRY(cx.fp1.ensure(Rn * 8));
        PW_TRY(cx.guniq.ensure(Rn * 4));
        PW_TRY(cx.rkey.ensure(Rn * 8));
        PW_TRY(cx.rkey_s.ensure(Rn * 8));
        PW_TRY(cx.ridx.ensure(Rn * 4));
        PW_TRY(cx.ridx_s.ensure(Rn * 4));
        PW_TRY(cx.first_run.ensure(Rn * 4));
        const u64 mask = cx.mask ? cx.mask : ~0ull;
        bool exact = false;
        for (int attempt = 0; attempt < kSeeds && !exact; ++attempt) {
            ++cx.stat_seeds;
            const u64 seed0 = mix64(0x626c6f636b73ull + (u64)attempt), seed1 = mix64(0x72756e73ull + 31 * (u64)attempt);
            {
                ScopedKernelTimer timer("execution_blocks_fingerprint");
                hipLaunchKernelGGL(execution_blocks_hash_kernel, dim3(div_up(K, kBlock)), dim3(kBlock), 0, st, d_S, d_rid, (const uint32_t*)rs.p, K, seed0, seed1,
                                   cx.h0.as<u64>(), cx.h1.as<u64>());
                PW_HIP_TRY(hipGetLastError());
                for (int half = 0; half < 2; ++half)
                    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                        return rocprim::reduce_by_key(t, b, d_rid, (half ? cx.h1 : cx.h0).as<u64>(), (unsigned int)K, cx.guniq.as<uint32_t>(), (half ? cx.fp1 : cx.fp0).as<u64>(),
                                                      d_n, rocprim::plus<u64>(), rocprim::equal_to<uint32_t>(), st);
                    }));
            }
            {
                ScopedKernelTimer timer("execution_blocks_group_runs");
                const dim3 grid(div_up(Rn, kBlock)), block(kBlock);
                hipLaunchKernelGGL(execution_blocks_runkey_kernel, grid, block, 0, st, (const u64*)cx.fp0.p, (const u64*)cx.fp1.p, (const uint32_t*)rs.p, Rn, mask,
                                   cx.rkey.as<u64>(), cx.ridx.as<uint32_t>());
                PW_HIP_TRY(hipGetLastError());
                PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                    return rocprim::radix_sort_pairs(t, b, cx.rkey.as<u64>(), cx.rkey_s.as<u64>(), cx.ridx.as<uint32_t>(), cx.ridx_s.as<uint32_t>(), (size_t)Rn, 0u, 64u, st);
                }));
                hipLaunchKernelGGL(execution_blocks_group_kernel, grid, block, 0, st, (const u64*)cx.rkey_s.p, Rn, cx.ridx.as<uint32_t>());
                PW_HIP_TRY(hipGetLastError());
                PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                    return rocprim::inclusive_scan(t, b, cx.ridx.as<uint32_t>(), cx.guniq.as<uint32_t>(), (size_t)Rn, rocprim::maximum<uint32_t>(), st);
                }));
                hipLaunchKernelGGL(execution_blocks_first_kernel, grid, block, 0, st, (const uint32_t*)cx.ridx_s.p, (const uint32_t*)cx.guniq.p, Rn, cx.first_run.as<uint32_t>());
            }
            {
                ScopedKernelTimer timer("execution_blocks_verify_kernel");
                PW_HIP_TRY(hipMemsetAsync(d_counters + 1, 0, 8, st));
                hipLaunchKernelGGL(execution_blocks_verify_kernel, dim3(div_up(K, kBlock)), dim3(kBlock), 0, st, d_S, d_rid, (const uint32_t*)rs.p,
                                   (const uint32_t*)cx.first_run.p, K, d_counters);
                PW_HIP_TRY(hipGetLastError());
                PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
                PW_HIP_TRY(hipStreamSynchronize(st));
            }
            exact = counters[1] == 0;
        }
        if (!exact) {
            *status = 6;
            return (int)hipGetLastError();
        }
        std::vector<uint32_t> h_first(Rn);
        PW_HIP_TRY(hipMemcpyAsync(h_first.data(), cx.first_run.p, Rn * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        for (Scratch::Buf* b : {&cx.h0, &cx.h1, &cx.fp0, &cx.fp1, &cx.guniq, &cx.rkey, &cx.rkey_s, &cx.ridx, &cx.ridx_s, &cx.first_run, &cx.sflag}) b->release();
        // the distinct runs with their counts, in the order of a map keyed by the start pcs (= by the block indices)
        std::vector<u64> times(Rn, 0);
        std::vector<uint32_t> distinct;
        for (u64 r = 0; r < Rn; ++r)
            if (!times[h_first[r]]++) distinct.push_back(h_first[r]);
        // sorted by (the first few blocks packed into one word, 0 = the run has ended: a prefix sorts first), then by the rest
        const unsigned slot = bits_for(n_blocks + 1), slots = 64 / slot;
        std::vector<std::pair<u64, uint32_t>> order;
        order.reserve(distinct.size());
        u64 total = 0;
        for (uint32_t r : distinct) {
            u64 key = 0;
            for (unsigned k = 0; k < slots; ++k) key = (key << slot) | (h_rs[r] + k < h_rs[r + 1] ? (u64)h_S[h_rs[r] + k] + 1 : 0);
            order.emplace_back(key, r);
            total += h_rs[r + 1] - h_rs[r];
        }
        std::sort(order.begin(), order.end(), [&](const std::pair<u64, uint32_t>& x, const std::pair<u64, uint32_t>& y) {
            if (x.first != y.first) return x.first < y.first;
            return std::lexicographical_compare(h_S.begin() + h_rs[x.second], h_S.begin() + h_rs[x.second + 1], h_S.begin() + h_rs[y.second],
                                                h_S.begin() + h_rs[y.second + 1]);
        });
        R.run_pcs.resize(total);
        R.run_off.reserve(order.size() + 1);
        R.run_counts.reserve(order.size());
        uint32_t* at = R.run_pcs.data();
        for (const auto& o : order) {
            const uint32_t r = o.second;
            for (u64 i = h_rs[r]; i < h_rs[r + 1]; ++i) *at++ = blocks[h_S[i]].start_pc;
            R.run_off.push_back((u64)(at - R.run_pcs.data()));
            R.run_counts.push_back(times[r]);
        }
    }

    // ---- levels ----
    if (K) {
        // windows of length L that fit their run: the sum over the runs of max(0, length - L + 1), from the runs' lengths capped at 256
        std::vector<u64> runs_of(258, 0), len_of(258, 0);
        for (u64 r = 0; r < n_runs; ++r) {
            const u64 len = h_rs[r + 1] - h_rs[r], c = std::min<u64>(len, 256);
            ++runs_of[c];
            len_of[c] += len;
        }
        for (int c = 256; c-- > 0;) {
            runs_of[c] += runs_of[c + 1];
            len_of[c] += len_of[c + 1];
        }
        const uint32_t* d_rs = cx.rs.as<uint32_t>();
        Scratch::Buf& pos_s = cx.pos_s;
        PW_TRY(cx.id_a.ensure(K * 4));
        PW_TRY(cx.id_b.ensure(K * 4));
        PW_TRY(cx.key.ensure(K * 8));
        PW_TRY(cx.key_s.ensure(K * 8));
        PW_TRY(cx.pos.ensure(K * 4));
        PW_TRY(pos_s.ensure(K * 4));
        PW_TRY(cx.hflag.ensure(K * 4));
        PW_TRY(cx.rank.ensure(K * 4));
        PW_TRY(cx.cval.ensure(K * 4));
        PW_TRY(cx.cstart.ensure(K * 4));
        PW_TRY(cx.val.ensure(K * 8));
        PW_TRY(cx.st_a.ensure(K * 8));
        PW_TRY(cx.st_b.ensure(K * 8));
        PW_TRY(cx.gkey.ensure(K * 8));
        PW_TRY(cx.gsum.ensure(K * 8));
        PW_TRY(cx.guniq.ensure(K * 4));
        const unsigned bbits = bits_for(n_blocks);
        struct Level { std::vector<u64> key, count; };
        std::vector<Level> levels;
        u64 groups_prev = 1;
        uint32_t *id_prev = cx.id_a.as<uint32_t>(), *id_next = cx.id_b.as<uint32_t>();
        for (uint32_t L = 1; L <= max_bb; ++L) {
            const u64 n_fit = L <= 256 ? len_of[L] - (u64)(L - 1) * runs_of[L] : 0;
            if (!n_fit) break;
            ++cx.stat_levels;
            const unsigned key_bits = L == 1 ? bbits : bits_for(groups_prev) + bbits;  // (31 + 32 at most), one more for `invalid`
            {
                ScopedKernelTimer timer("execution_blocks_name_sort");
                hipLaunchKernelGGL(execution_blocks_key_kernel, dim3(div_up(K, kBlock)), dim3(kBlock), 0, st, d_S, d_rid, d_rs, (const uint32_t*)id_prev, K, L, bbits,
                                   (u64)1 << key_bits, cx.key.as<u64>(), cx.pos.as<uint32_t>());
                PW_HIP_TRY(hipGetLastError());
                PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                    return rocprim::radix_sort_pairs(t, b, cx.key.as<u64>(), cx.key_s.as<u64>(), cx.pos.as<uint32_t>(), pos_s.as<uint32_t>(), (size_t)K, 0u, key_bits + 1, st);
                }));
            }
            {
                ScopedKernelTimer timer("execution_blocks_greedy_count");
                PW_HIP_TRY(hipMemsetAsync(d_counters + 3, 0, 8, st));
                PW_TRY(greedy_chains(cx, (const u64*)cx.key_s.p, (const uint32_t*)pos_s.p, n_fit, L, cx.hflag.as<uint32_t>(), cx.rank.as<uint32_t>(), id_next, d_counters,
                                     nullptr, nullptr));
                PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                    return rocprim::reduce_by_key(t, b, cx.rank.as<uint32_t>(), cx.val.as<u64>(), (unsigned int)n_fit, cx.guniq.as<uint32_t>(), cx.gsum.as<u64>(), d_n,
                                                  rocprim::plus<u64>(), rocprim::equal_to<uint32_t>(), st);
                }));
                PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
                    return rocprim::select(t, b, cx.key_s.as<u64>(), cx.hflag.as<uint32_t>(), cx.gkey.as<u64>(), d_n + 1, (size_t)n_fit, st);
                }));
                PW_HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof counters, hipMemcpyDeviceToHost, st));
                PW_HIP_TRY(hipStreamSynchronize(st));
            }
            const u64 G = (uint32_t)counters[4];
            if (G != (uint32_t)(counters[4] >> 32)) return (int)hipErrorInvalidValue;
            cx.stat_jumping += counters[3];
            Level lv;
            lv.key.resize(G);
            lv.count.resize(G);
            PW_HIP_TRY(hipMemcpyAsync(lv.key.data(), cx.gkey.p, G * 8, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipMemcpyAsync(lv.count.data(), cx.gsum.p, G * 8, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            levels.push_back(std::move(lv));
            groups_prev = G;
            std::swap(id_prev, id_next);
        }
        // The names of a level ascend with the windows' lexicographic order, and a window's extensions are contiguous in the next
        // level (sorted by the name of their first L - 1 blocks): a walk in preorder writes the map's order, a prefix before its
        // extensions.
        const u64 low = ((u64)1 << bbits) - 1;
        std::vector<u64> at(levels.size() + 1, 0);  // the next unread window of every level
        std::vector<uint32_t> path;
        struct Frame { size_t level; u64 g; };
        std::vector<Frame> stack;
        {
            size_t windows = 0, elements = 0;
            for (size_t l = 0; l < levels.size(); ++l) {
                windows += levels[l].key.size();
                elements += levels[l].key.size() * (l + 1);
            }
            R.sb_pcs.reserve(elements);
            R.sb_off.reserve(windows + 1);
            R.sb_counts.reserve(windows);
        }
        for (u64 g0 = 0; g0 < (levels.empty() ? 0 : levels[0].key.size()); ++g0) {
            stack.push_back(Frame{0, g0});
            while (!stack.empty()) {
                const Frame f = stack.back();
                const Level& lv = levels[f.level];
                if (path.size() == f.level) {  // first visit: write the window
                    path.push_back(blocks[lv.key[f.g] & low].start_pc);
                    R.sb_pcs.insert(R.sb_pcs.end(), path.begin(), path.end());
                    R.sb_off.push_back(R.sb_pcs.size());
                    R.sb_counts.push_back(lv.count[f.g]);
                }
                const size_t nl = f.level + 1;
                if (nl < levels.size() && at[nl] < levels[nl].key.size() && (levels[nl].key[at[nl]] >> bbits) == f.g) {
                    stack.push_back(Frame{nl, at[nl]++});
                } else {
                    path.pop_back();
                    stack.pop_back();
                }
            }
        }
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pw_execution_blocks_from_pcs(const uint32_t* d_pcs, uint64_t n, uint32_t pc_step, const PwBasicBlock* blocks, size_t n_blocks, uint32_t max_bb,
                                            size_t scratch_bytes, PwExecutionBlocks** out, uint32_t* status, uint64_t* info) {
    if (!out || !status || !info || (!d_pcs && n) || !pc_step || !max_bb || max_bb > 255u || n >= ((uint64_t)1 << 32) ||
        !time_index::blocks_well_formed(blocks, n_blocks, pc_step))
        return -1;
    EbCtx& cx = g_eb;
    const ScratchCall call(cx, out, status, info);
    auto result = empty_result(blocks, n_blocks);
    if (!n) {
        *out = result.release();
        return 0;
    }
    const int rc = detect_blocks(cx, d_pcs, nullptr, n, pc_step, blocks, n_blocks, max_bb, call.bound(scratch_bytes), 0, result, status, info);
    if (!rc && !*status) *out = result.release();
    return rc;
}

extern "C" int pw_execution_blocks_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, uint32_t pc_step,
                                               const PwBasicBlock* blocks, size_t n_blocks, uint32_t max_bb, size_t scratch_bytes, PwExecutionBlocks** out,
                                               uint32_t* status, uint64_t* info) {
    if (!out || !status || !info || !pc_step || !max_bb || max_bb > 255u || bus >= bb::P || !airs_well_formed(airs, n_airs) ||
        !time_index::blocks_well_formed(blocks, n_blocks, pc_step))
        return -1;
    time_index::Bridge B;
    if (!time_index::bridge_of(airs, n_airs, bus, &B) || B.M >= ((u64)1 << 32)) return -1;
    const u64 M = B.M;
    EbCtx& cx = g_eb;
    const ScratchCall call(cx, out, status, info);
    auto result = empty_result(blocks, n_blocks);
    if (!M) {
        *out = result.release();
        return 0;
    }
    const size_t bound = call.bound(scratch_bytes);
    // the index stage holds 32 bytes per row and a sort's temporary storage; the sorted keys and pcs stay through the heads stage
    const size_t index_need = time_index::bytes_needed(M), extra = 64 + (size_t)M * 12;
    if (bound < index_need) {
        *status = 2;
        *info = std::max({index_need, heads_need(M) + extra, levels_need(M)});  // (what is known before a row is read)
        return 0;
    }
    u64 N = 0;
    PW_TRY(time_index::open(airs, segment_of_air, n_airs, bus, B, cx.index, cx.temp,
                            time_index::Names{"execution_blocks_index_kernel", "execution_blocks_sort_time", "execution_blocks_time_kernel"}, &N, status, info));
    if (*status) return (int)hipGetLastError();
    if (!N) {
        *out = result.release();
        return (int)hipGetLastError();
    }
    cx.index.release_except({&cx.index.icount, &cx.index.tkey_s, &cx.index.pc_t});  // (`extra` above: the counters' 64 bytes and 12 per row)
    cx.temp.release();
    const int rc = detect_blocks(cx, (const uint32_t*)cx.index.pc_t.p, (const u64*)cx.index.tkey_s.p, N, pc_step, blocks, n_blocks, max_bb, bound, extra, result, status, info);
    if (!rc && !*status) *out = result.release();
    return rc;
}

extern "C" int pw_execution_blocks_count(PwExecutionBlocks* e, const uint32_t* needle_start_pcs, uint32_t len, int remove, uint64_t* count) {
    if (!e || !count || !len || !needle_start_pcs) return -1;
    *count = 0;
    const u64 K = e->K;
    if (!K || len > K) return 0;
    std::vector<uint32_t> needle(len);
    for (uint32_t k = 0; k < len; ++k) {
        const auto at = std::lower_bound(e->blocks.begin(), e->blocks.end(), needle_start_pcs[k], [](const PwBasicBlock& b, uint32_t pc) { return b.start_pc < pc; });
        if (at == e->blocks.end() || at->start_pc != needle_start_pcs[k]) return 0;
        needle[k] = (uint32_t)(at - e->blocks.begin());
    }
    EbCtx& cx = g_eb;
    const ScratchCall call(cx, ScratchCall::kContinues);
    DeviceBuf tables;
    hipStream_t st = stream();
    const size_t off_needle = 64;
    PW_TRY(cx.small.ensure(off_needle + (size_t)len * 4));
    u64* d_counters = cx.small.as<u64>();
    uint32_t* d_needle = (uint32_t*)(cx.small.as<char>() + off_needle);
    uint32_t* d_n = (uint32_t*)(d_counters + 4);
    PW_HIP_TRY(hipMemsetAsync(d_counters, 0, 64, st));
    PW_HIP_TRY(hipMemcpyAsync(d_needle, needle.data(), (size_t)len * 4, hipMemcpyHostToDevice, st));
    ScopedKernelTimer timer("execution_blocks_count");
    PW_TRY(cx.hflag.ensure(K * 4));
    PW_TRY(cx.pos.ensure(K * 4));
    hipLaunchKernelGGL(execution_blocks_match_kernel, dim3(div_up(K, kBlock)), dim3(kBlock), 0, st, (const uint32_t*)e->S.p, (const uint32_t*)e->rid.p, K,
                       (const uint32_t*)d_needle, len, cx.hflag.as<uint32_t>());
    PW_HIP_TRY(hipGetLastError());
    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
        return rocprim::select(t, b, rocprim::counting_iterator<uint32_t>(0), cx.hflag.as<uint32_t>(), cx.pos.as<uint32_t>(), d_n, (size_t)K, st);
    }));
    uint32_t n32 = 0;
    PW_HIP_TRY(hipMemcpyAsync(&n32, d_n, 4, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    const u64 n = n32;
    if (!n) return (int)hipGetLastError();
    PW_TRY(cx.cval.ensure(n * 4));
    PW_TRY(cx.cstart.ensure(n * 4));
    PW_TRY(cx.val.ensure(n * 8));
    PW_TRY(cx.st_a.ensure(n * 8));
    PW_TRY(cx.st_b.ensure(n * 8));
    int rounds = 0;
    PW_TRY(greedy_chains(cx, nullptr, (const uint32_t*)cx.pos.p, n, len, nullptr, nullptr, nullptr, d_counters, remove ? &tables : nullptr, &rounds));
    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::reduce(t, b, cx.val.as<u64>(), d_counters + 5, (u64)0, (size_t)n, rocprim::plus<u64>(), st); }));
    u64 total = 0;
    PW_HIP_TRY(hipMemcpyAsync(&total, d_counters + 5, 8, hipMemcpyDeviceToHost, st));
    if (remove) {
        uint32_t* chosen = cx.hflag.as<uint32_t>();  // (n <= K words)
        const dim3 grid(div_up(n, kBlock)), block(kBlock);
        hipLaunchKernelGGL(execution_blocks_chosen_kernel, grid, block, 0, st, (const uint32_t*)cx.cstart.p, n, chosen);
        for (int k = rounds; k-- > 0;) hipLaunchKernelGGL(execution_blocks_mark_kernel, grid, block, 0, st, (const u64*)(tables.as<u64>() + (size_t)k * n), n, chosen);
        hipLaunchKernelGGL(execution_blocks_remove_kernel, dim3(div_up(n * len, kBlock)), block, 0, st, (const uint32_t*)cx.pos.p, (const uint32_t*)chosen, n, len,
                           e->S.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
    }
    PW_HIP_TRY(hipStreamSynchronize(st));
    *count = total;
    return (int)hipGetLastError();
}
