// Cutting one execution into segments on the device under APC-aware limits (include/powdr_prover.h pw_execution_segments_from_traces,
// DESIGN.md §5v): from the instruction-AIR traces of one long execution and (optionally) the calls chosen for it, the greedy cut
// b_0 = 0 < b_1 < .. < b_S = N in which every segment is as long as the height cap and the cell budget allow and no call is cut,
// per segment its first time key and pc, its calls, its class counts, and per (segment, AIR) the row list pw_trace_gather_rows takes.
//   index      time_index.hpp, unchanged: position i < N is the active row with the i-th smallest time key, idx_s[i] its global row
//   classify   execution_segments_classify_kernel   one lane per position: its AIR from the global row number, its call by binary
//                                                   search in the call table; key = AIR * 2 + covered
//   sort       rocPRIM radix sort (stable) of (key, position) over the key bits in use: per AIR the ascending list of its uncovered
//                                                   positions (an AIR class) and of its covered ones. The list of an APC class is
//                                                   the starts of its calls (host: the call table is sorted). cnt_c(p, q) is two
//                                                   lower bounds in the class's list.
//   bounds     execution_segments_bounds_kernel     ONE workgroup loops over the segments, lanes striding over the classes (class c
//                                                   is always lane c % 256's, which keeps a cursor = lower bound of b_s per class).
//                                                   Height bound: min over the classes of the position of the (cap + 1)-th element
//                                                   from the cursor. Cell bound: bisection over q with one workgroup sum per probe.
//                                                   A bound strictly inside a call snaps down to the call's start.
//   heights    execution_segments_heights_kernel    one lane per (segment, class)
//   lists      execution_segments_rows_kernel       one lane per (segment, AIR): its rows and the AIR's rank at b_s
//              (host)                               the lists' places: padded(rows) words each, 16-byte aligned; cleared to 0xFFFFFFFF
//              execution_segments_scatter_kernel    one lane per position writes its row at its rank in the list of its (segment, AIR)
// Nothing depends on an order of arrival: every output word has one writer, and the sort is stable.
// With a meter (pw_execution_segments_from_traces_metered) the bounds stage becomes a loop over the segments driven from
// the host, in which the distinct memory blocks and Merkle nodes of the candidate segment are further limits: "the system meter" below.
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

#include <memory>

namespace pw {

namespace {

using namespace bus;

constexpr u64 kSat = ~0ull;                      // a saturated cell count
constexpr u64 kDefaultMaxSegments = 1ull << 20;  // max_segments == 0
constexpr size_t kHeightChunk = (size_t)1 << 20; // (segment, class) pairs per launch of the heights kernel

// the first index in [lo, hi) with a[i] >= q (hi if none)
__device__ __forceinline__ u64 lower_bound_u32(const uint32_t* __restrict__ a, u64 lo, u64 hi, u64 q) {
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((u64)a[mid] < q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the number of entries of the ascending table t[0 .. n) that are <= q
__device__ __forceinline__ u64 upper_bound_u64(const u64* __restrict__ t, u64 n, u64 q) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if (t[mid] <= q) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__host__ __device__ __forceinline__ u64 padded_height(u64 n, u64 min_h) {
    if (!n) return 0;
    u64 p = 1;
    while (p < n) p <<= 1;
    return p < min_h ? min_h : p;
}

__host__ __device__ __forceinline__ u64 sat_add(u64 a, u64 b) {
    const u64 s = a + b;
    return s < a ? kSat : s;
}

// key[p] = part * 2 + covered, pos[p] = p
__global__ __launch_bounds__(kBlock) void execution_segments_classify_kernel(const uint32_t* __restrict__ idx_s, const u64* __restrict__ part_g0, uint32_t n_parts,
                                                                              const u64* __restrict__ from, const u64* __restrict__ to, uint32_t n_calls, u64 N,
                                                                              uint32_t* __restrict__ key, uint32_t* __restrict__ pos) {
    const u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (p >= N) return;
    const u64 g = idx_s[p];
    uint32_t lo = 0, hi = n_parts;  // the last part with g0 <= g
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (part_g0[mid] <= g) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t part = lo - 1;
    const u64 j = upper_bound_u64(from, n_calls, p);  // the calls that start at or before p
    const uint32_t covered = j && p < to[j - 1] ? 1u : 0u;
    key[p] = part * 2u + covered;
    pos[p] = (uint32_t)p;
}

// kstart[k] = the first sorted index with key >= k, k = 0 .. n_keys
__global__ void execution_segments_starts_kernel(const uint32_t* __restrict__ key_s, u64 N, uint32_t n_keys, u64* __restrict__ kstart) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k <= n_keys) kstart[k] = lower_bound_u32(key_s, 0, N, k);
}

// the list of class c in cpos: an AIR class's uncovered positions (from the sort), an APC class's call starts (cpos[N ..], from the host)
__global__ void execution_segments_classes_kernel(const u64* __restrict__ kstart, const u64* __restrict__ astart, uint32_t n_parts, uint32_t n_apcs, u64 N,
                                                  u64* __restrict__ cbeg, u64* __restrict__ cend) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < n_parts) {
        cbeg[c] = kstart[2 * c];
        cend[c] = kstart[2 * c + 1];
    } else if (c < n_parts + n_apcs) {
        cbeg[c] = N + astart[c - n_parts];
        cend[c] = N + astart[c - n_parts + 1];
    }
}

struct BoundsArgs {
    const uint32_t* cpos;
    const u64* cbeg;
    const u64* cend;
    const u64* cwidth;
    u64* ccur;  // per class: the lower bound of b_s in its list
    const u64* from;
    const u64* to;
    u64* bounds;  // [max_segments + 1]
    u64* result;  // [0] S | [1] status | [2] info | [3] cell-bound probes | [4] cuts snapped to a call's start
    u64 N, cap, min_h, max_cells, max_segments;
    uint32_t n_classes, n_calls;
};

__device__ __forceinline__ u64 block_min(u64 v, u64* sh) {
    v = wave_min(v);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = sh[w] < r ? sh[w] : r;
    __syncthreads();
    return r;
}

__device__ __forceinline__ u64 block_sat_sum(u64 v, u64* sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = sat_add(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    u64 r = sh[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) r = sat_add(r, sh[w]);
    __syncthreads();
    return r;
}

// sum_c width_c * padded(cnt_c(b, q)) for a q at or below the height bound (so no count passes the cap), saturating
__device__ __forceinline__ u64 cells_upto(const BoundsArgs& a, u64 q, u64* sh) {
    u64 sum = 0;
    for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) {
        const u64 i0 = a.ccur[c], end = a.cend[c], hi = end - i0 > a.cap ? i0 + a.cap + 1 : end;
        const u64 cnt = lower_bound_u32(a.cpos, i0, hi, q) - i0;
        sum = sat_add(sum, a.cwidth[c] * padded_height(cnt, a.min_h));  // (width < 2^32, padded <= 2^31)
    }
    return block_sat_sum(sum, sh);
}

// one workgroup; every lane follows the same b, q and s (the reductions broadcast)
__global__ __launch_bounds__(kBlock) void execution_segments_bounds_kernel(BoundsArgs a) {
    __shared__ u64 sh[kWaves];
    for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) a.ccur[c] = a.cbeg[c];
    u64 b = 0, s = 0, probes = 0, snapped = 0, status = 0, info = 0;
    if (threadIdx.x == 0u) a.bounds[0] = 0;
    while (b < a.N) {
        if (s == a.max_segments) {
            status = 14;
            info = b;
            break;
        }
        // the height bound: the smallest position at which a class holds cap + 1 elements from b on
        u64 hb = a.N;
        for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) {
            const u64 i0 = a.ccur[c];
            if (a.cend[c] - i0 > a.cap) {
                const u64 at = a.cpos[i0 + a.cap];
                hb = at < hb ? at : hb;
            }
        }
        hb = block_min(hb, sh);
        u64 q = hb;
        if (a.max_cells) {
            ++probes;
            if (cells_upto(a, hb, sh) > a.max_cells) {
                u64 lo = b, hi = hb;  // fits(b, lo), not fits(b, hi)
                while (hi - lo > 1) {
                    const u64 mid = lo + (hi - lo) / 2;
                    ++probes;
                    if (cells_upto(a, mid, sh) <= a.max_cells) lo = mid;
                    else hi = mid;
                }
                q = lo;
            }
        }
        if (q > b && a.n_calls) {  // strictly inside a call: down to its start
            const u64 j = upper_bound_u64(a.from, a.n_calls, q - 1);  // the calls with from < q
            if (j && q < a.to[j - 1]) {
                q = a.from[j - 1];
                ++snapped;
            }
        }
        if (q <= b) {
            status = 13;
            info = b;
            break;
        }
        for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) a.ccur[c] = lower_bound_u32(a.cpos, a.ccur[c], a.cend[c], q);
        ++s;
        if (threadIdx.x == 0u) a.bounds[s] = q;
        b = q;
    }
    if (threadIdx.x == 0u) {
        a.result[0] = s;
        a.result[1] = status;
        a.result[2] = info;
        a.result[3] = probes;
        a.result[4] = snapped;
    }
}

// tkey[s], pc[s] of position b_s
__global__ __launch_bounds__(kBlock) void execution_segments_first_kernel(const u64* __restrict__ bounds, u64 S, const u64* __restrict__ tkey_s,
                                                                           const uint32_t* __restrict__ pc_t, u64* __restrict__ tkey, uint32_t* __restrict__ pc) {
    const u64 s = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (s >= S) return;
    tkey[s] = tkey_s[bounds[s]];
    pc[s] = pc_t[bounds[s]];
}

// out[(s - s0) * n_classes + c] = cnt_c(b_s, b_(s+1)) for s0 <= s < s1
__global__ __launch_bounds__(kBlock) void execution_segments_heights_kernel(const uint32_t* __restrict__ cpos, const u64* __restrict__ cbeg, const u64* __restrict__ cend,
                                                                             uint32_t n_classes, const u64* __restrict__ bounds, u64 s0, u64 s1,
                                                                             uint32_t* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (s1 - s0) * n_classes) return;
    const u64 s = s0 + i / n_classes;
    const uint32_t c = (uint32_t)(i % n_classes);
    const u64 lo = lower_bound_u32(cpos, cbeg[c], cend[c], bounds[s]);
    out[i] = (uint32_t)(lower_bound_u32(cpos, lo, cend[c], bounds[s + 1]) - lo);
}

// per (segment, part): the part's positions before b_s (covered ones included) and those in [b_s, b_(s+1))
__global__ __launch_bounds__(kBlock) void execution_segments_rows_kernel(const uint32_t* __restrict__ cpos, const u64* __restrict__ kstart, uint32_t n_parts,
                                                                          const u64* __restrict__ bounds, u64 S, uint32_t* __restrict__ base, uint32_t* __restrict__ rows) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= S * n_parts) return;
    const u64 s = i / n_parts;
    const uint32_t k = (uint32_t)(i % n_parts);
    const u64 u0 = kstart[2 * k], u1 = kstart[2 * k + 1], c1 = kstart[2 * k + 2];
    const u64 before = (lower_bound_u32(cpos, u0, u1, bounds[s]) - u0) + (lower_bound_u32(cpos, u1, c1, bounds[s]) - u1);
    const u64 upto = (lower_bound_u32(cpos, u0, u1, bounds[s + 1]) - u0) + (lower_bound_u32(cpos, u1, c1, bounds[s + 1]) - u1);
    base[i] = (uint32_t)before;
    rows[i] = (uint32_t)(upto - before);
}

// sorted index i: position p of part k = key / 2; its rank among the part's positions = its rank in its own list + the entries of the
// part's other list before p
__global__ __launch_bounds__(kBlock) void execution_segments_scatter_kernel(const uint32_t* __restrict__ key_s, const uint32_t* __restrict__ cpos,
                                                                             const u64* __restrict__ kstart, const uint32_t* __restrict__ idx_s,
                                                                             const u64* __restrict__ part_g0, uint32_t n_parts, const u64* __restrict__ bounds, u64 S,
                                                                             const uint32_t* __restrict__ base, const u64* __restrict__ list_off, u64 N,
                                                                             uint32_t* __restrict__ lists) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= N) return;
    const uint32_t key = key_s[i], k = key >> 1, other = key ^ 1u;
    const u64 p = cpos[i];
    const u64 s = upper_bound_u64(bounds, S + 1, p) - 1;  // (b_0 = 0 <= p < N = b_S: 0 <= s < S)
    const u64 o0 = kstart[other], o1 = kstart[other + 1];
    const u64 rank = (i - kstart[key]) + (lower_bound_u32(cpos, o0, o1, p) - o0) - base[s * n_parts + k];
    lists[list_off[s * n_parts + k] + rank] = (uint32_t)((u64)idx_s[p] - part_g0[k]);
}

// ---- the system meter: the distinct memory blocks and Merkle nodes of a candidate segment as limits of the cut ----
//   walk     execution_meter_walk_kernel    one lane per row of every participating AIR on the memory bus: an access of the row at
//                                           position p is appended as (p << 32 | key), one counter add per wave and interaction
//   sort     rocPRIM radix sort of the 64-bit words: by position, then key (equal words are equal accesses: nothing downstream
//                                           depends on the order of arrival); execution_meter_starts_kernel: astart[p] = the
//                                           first access at a position >= p, so a window of positions is a range of accesses
//   tiles    per segment from b_s, in ascending tiles of positions up to the class height bound:
//            execution_meter_insert_kernel  one lane per access walks up from level 0: atomicMin(first[(l, key >> l)], position << 32
//                                           | access index), stopping at the first node that held a smaller word (its owner carries
//                                           that word on upward, so the minimum reaches every ancestor)
//            execution_meter_count_kernel   the owner of a node's `first` adds 1 to dM[position] (at level 0 also to dB): a later
//                                           tile never lowers an earlier tile's word, so only the nodes new in this tile count
//            execution_meter_scan_kernel    one workgroup: the prefixes B(b, q), M(b, q) of the tile's positions and the first
//                                           position at which one passes its cap
//   bounds   execution_meter_close_kernel   one workgroup, §5v's step for ONE segment: the smaller of the class height bound and the
//                                           system bound, the cell bisection with the three system terms by prefix look-up, the snap
//                                           into calls, the cursors; and the next segment's class height bound
// Integer atomics on unique owners: the counts do not depend on the order of arrival, nor on the tile or the table size.
constexpr u64 kDefaultMeterTile = 1ull << 14;  // positions per tile
constexpr uint32_t kNoPos = 0xffffffffu;
constexpr size_t kNodeSlotBytes = 16;  // node 8, first 8
constexpr uint32_t kMemoryArgs = 7;    // as, ptr, four data words, timestamp
constexpr uint32_t kPtrBits = 29;

struct NodeTable { TableView v; u64* first; };

__global__ __launch_bounds__(kBlock) void execution_meter_positions_kernel(const uint32_t* __restrict__ idx_s, u64 N, uint32_t* __restrict__ pos_of_row) {
    const u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (p < N) pos_of_row[idx_s[p]] = (uint32_t)p;
}

// counters: [0] accesses appended | [1] the smallest witness of an access without a key
// Every loop is wave-uniform (a lane without a position carries no access), so that the lanes of a wave share one counter add.
template <bool FAST>
__global__ __launch_bounds__(kBlock) void execution_meter_walk_kernel(const uint32_t* __restrict__ m, size_t H, LogupProgram lp, const uint32_t* __restrict__ order,
                                                                       uint32_t begin, uint32_t end, uint32_t air, u64 g0, const uint32_t* __restrict__ pos_of_row,
                                                                       uint32_t tree_height, u64* __restrict__ acc, u64 cap, u64* __restrict__ counters) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const unsigned lane = threadIdx.x & 63u;
    const uint32_t p = r < H ? pos_of_row[g0 + r] : kNoPos;
    u64 bad = kEmpty;
    for (uint32_t i = begin; i < end; ++i) {
        const uint32_t idx = order[i];
        const LogupInteraction it = lp.d_inter[idx];
        bool have = false;
        u64 key = 0;
        if (p != kNoPos && eval_span<FAST>(lp, it.first_span, m, H, r, stk) != 0u) {
            const uint32_t as = bb::from_monty(eval_span<FAST>(lp, it.first_span + 1, m, H, r, stk));
            const uint32_t ptr = bb::from_monty(eval_span<FAST>(lp, it.first_span + 2, m, H, r, stk));
            key = ((u64)(as - 1u) << kPtrBits) + (u64)ptr;
            have = as - 1u < 2u && ptr < (1u << kPtrBits) && (key >> tree_height) == 0ull;
            if (!have) {
                const u64 w = pack_witness(air, idx, r);
                bad = w < bad ? w : bad;
            }
        }
        const u64 havers = __builtin_amdgcn_ballot_w64(have);
        if (havers) {
            const int leader = __builtin_ctzll(havers);
            u64 base = 0;
            if ((int)lane == leader) base = atomicAdd(counters, (u64)__builtin_popcountll(havers));
            base = __shfl(base, leader, 64);
            const u64 at = base + (u64)__builtin_popcountll(havers & ((1ull << lane) - 1ull));
            if (have && at < cap) acc[at] = ((u64)p << 32) | key;  // (cap holds every interaction of every row)
        }
    }
    if (__builtin_amdgcn_ballot_w64(bad != kEmpty)) {  // (never on honest traces)
        const u64 w = wave_min(bad);
        if (lane == 0u) atomicMin(counters + 1, w);
    }
}

// astart[p] = the first sorted access at a position >= p, p = 0 .. N
__global__ __launch_bounds__(kBlock) void execution_meter_starts_kernel(const u64* __restrict__ acc_s, u64 A, u64 N, uint32_t* __restrict__ astart) {
    const u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (p > N) return;
    u64 lo = 0, hi = A;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2;
        if ((acc_s[mid] >> 32) < p) lo = mid + 1;
        else hi = mid;
    }
    astart[p] = (uint32_t)lo;
}

__device__ __forceinline__ u64 node_of(uint32_t level, uint32_t key) { return ((u64)level << 32) | (u64)(key >> level); }

// the accesses at the positions [lo, hi): lane i of the grid has access astart[lo] + i
__global__ __launch_bounds__(kBlock) void execution_meter_insert_kernel(const u64* __restrict__ acc_s, const uint32_t* __restrict__ astart, u64 lo, u64 hi,
                                                                         uint32_t tree_height, NodeTable t, uint32_t* __restrict__ overflow) {
    const u64 i = (u64)astart[lo] + (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (u64)astart[hi] || __atomic_load_n(overflow, __ATOMIC_RELAXED)) return;
    const u64 v = acc_s[i], mine = (v & ~0xffffffffull) | i;
    const uint32_t key = (uint32_t)v;
    for (uint32_t l = 0; l <= tree_height; ++l) {
        const u64 s = claim_slot<1>(t.v, node_of(l, key), 0, overflow);
        if (s == kEmpty) return;
        // (`first` only falls: a word at or below mine now stays there, and whoever set it walks on from here)
        if (__atomic_load_n(t.first + s, __ATOMIC_RELAXED) <= mine || atomicMin(t.first + s, mine) <= mine) break;
    }
}

// dB[p - lo], dM[p - lo] += the blocks and nodes whose `first` is an access at position p of the tile: the owner of a node owns every
// node below it on its own path, so a lane stops at the first level it does not own
__global__ __launch_bounds__(kBlock) void execution_meter_count_kernel(const u64* __restrict__ acc_s, const uint32_t* __restrict__ astart, u64 lo, u64 hi,
                                                                        uint32_t tree_height, NodeTable t, const uint32_t* __restrict__ overflow,
                                                                        uint32_t* __restrict__ dB, uint32_t* __restrict__ dM) {
    const u64 i = (u64)astart[lo] + (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (u64)astart[hi] || *overflow) return;
    const u64 v = acc_s[i], mine = (v & ~0xffffffffull) | i;
    const uint32_t key = (uint32_t)v;
    uint32_t n = 0;
    for (uint32_t l = 0; l <= tree_height; ++l) {
        const u64 s = find_slot(t.v, node_of(l, key));
        if (s == kEmpty || t.first[s] != mine) break;
        ++n;
    }
    if (n) {
        atomicAdd(dM + ((v >> 32) - lo), n);
        atomicAdd(dB + ((v >> 32) - lo), 1u);
    }
}

// One workgroup. PB[q - b], PM[q - b] = B(b, q), M(b, q) for q in (lo, hi] from the tile's deltas (cleared for the next tile) and
// the running sums in counts[0], counts[1] (a segment's first tile, lo == b, starts them); counts[2] = 1 + the first position p at
// which B(b, p + 1) > cap_b or M(b, p + 1) > cap_m, 0 while there is none. A table that overflowed leaves nothing but cleared deltas.
__global__ __launch_bounds__(kBlock) void execution_meter_scan_kernel(uint32_t* __restrict__ dB, uint32_t* __restrict__ dM, u64 b, u64 lo, u64 hi, u64 cap_b, u64 cap_m,
                                                                       u64* __restrict__ PB, u64* __restrict__ PM, u64* __restrict__ counts,
                                                                       const uint32_t* __restrict__ overflow) {
    __shared__ u64 sh_b[kWaves], sh_m[kWaves], sh[kWaves];
    const bool over = *overflow != 0u;
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    u64 run_b = lo == b ? 0 : counts[0], run_m = lo == b ? 0 : counts[1], bad = kEmpty;
    if (lo == b && threadIdx.x == 0u) PB[0] = PM[0] = 0;
    for (u64 base = lo; base < hi; base += kBlock) {
        const u64 j = base + threadIdx.x;
        u64 vb = 0, vm = 0;
        if (j < hi) {
            vb = dB[j - lo];
            vm = dM[j - lo];
            dB[j - lo] = 0;
            dM[j - lo] = 0;
        }
        if (over) continue;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const u64 ob = __shfl_up(vb, d, 64), om = __shfl_up(vm, d, 64);
            if ((int)lane >= d) {
                vb += ob;
                vm += om;
            }
        }
        if (lane == 63u) {
            sh_b[wave] = vb;
            sh_m[wave] = vm;
        }
        __syncthreads();
        u64 tot_b = 0, tot_m = 0;
#pragma unroll
        for (unsigned w = 0; w < (unsigned)kWaves; ++w) {
            if (w < wave) {
                vb += sh_b[w];
                vm += sh_m[w];
            }
            tot_b += sh_b[w];
            tot_m += sh_m[w];
        }
        __syncthreads();
        if (j < hi) {
            PB[j - b + 1] = run_b + vb;
            PM[j - b + 1] = run_m + vm;
            if ((run_b + vb > cap_b || run_m + vm > cap_m) && j < bad) bad = j;
        }
        run_b += tot_b;
        run_m += tot_m;
    }
    bad = block_min(bad, sh);
    if (threadIdx.x == 0u && !over) {
        counts[0] = run_b;
        counts[1] = run_m;
        counts[2] = bad == kEmpty ? 0 : bad + 1;
    }
}

__host__ __device__ __forceinline__ u64 padded_sys(u64 n, u64 min_h) {
    const u64 p = padded_height(n, min_h);
    return n && p < 2 ? 2 : p;
}

// the class height bound from the cursors: the smallest position at which a class holds cap + 1 elements from b on
__device__ __forceinline__ u64 class_bound(const BoundsArgs& a, u64* sh) {
    u64 hb = a.N;
    for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) {
        const u64 i0 = a.ccur[c];
        if (a.cend[c] - i0 > a.cap) {
            const u64 at = a.cpos[i0 + a.cap];
            hb = at < hb ? at : hb;
        }
    }
    return block_min(hb, sh);
}

// out[7] = the class height bound of the segment that starts at position 0
__global__ __launch_bounds__(kBlock) void execution_meter_open_kernel(BoundsArgs a, u64* __restrict__ out) {
    __shared__ u64 sh[kWaves];
    for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) a.ccur[c] = a.cbeg[c];
    __syncthreads();
    const u64 hb = class_bound(a, sh);
    if (threadIdx.x == 0u) {
        a.bounds[0] = 0;
        out[7] = hb;
    }
}

// sum_c width_c * padded(cnt_c(b, q)) + sum_k sys_width[k] * padded_sys(count_k(b, q)), saturating
__device__ __forceinline__ u64 cells_sys_upto(const BoundsArgs& a, u64 b, u64 q, const u64* __restrict__ PB, const u64* __restrict__ PM, const u64* sys_width, u64* sh) {
    u64 sum = cells_upto(a, q, sh);
    const u64 nb = PB[q - b], nm = PM[q - b];
    const u64 count[3] = {nb, nm, 2 * nm};
#pragma unroll
    for (int k = 0; k < 3; ++k)
        if (sys_width[k]) sum = sat_add(sum, sys_width[k] * padded_sys(count[k], a.min_h));  // (width < 2^32, padded <= 2^32)
    return sum;
}

struct CloseArgs {
    BoundsArgs a;
    const u64 *PB, *PM;  // the prefixes of the window that starts at b, valid up to q_max
    u64 b, s, q_max;     // q_max: the smaller of the class height bound and the first position that passes a system cap
    u64 sys_width[3];
    u64* out;            // [0] b_(s+1) | [1] status | [2] info | [3] probes | [4] snapped | [5] B | [6] M | [7] the next class height bound
};

// one workgroup; every lane follows the same q (the reductions broadcast)
__global__ __launch_bounds__(kBlock) void execution_meter_close_kernel(CloseArgs g) {
    __shared__ u64 sh[kWaves];
    const BoundsArgs& a = g.a;
    const u64 b = g.b;
    u64 q = g.q_max, probes = 0, snapped = 0, status = 0, info = 0;
    if (a.max_cells && q > b) {
        ++probes;
        if (cells_sys_upto(a, b, q, g.PB, g.PM, g.sys_width, sh) > a.max_cells) {
            u64 lo = b, hi = q;  // fits_sys(b, lo), not fits_sys(b, hi)
            while (hi - lo > 1) {
                const u64 mid = lo + (hi - lo) / 2;
                ++probes;
                if (cells_sys_upto(a, b, mid, g.PB, g.PM, g.sys_width, sh) <= a.max_cells) lo = mid;
                else hi = mid;
            }
            q = lo;
        }
    }
    if (q > b && a.n_calls) {  // strictly inside a call: down to its start
        const u64 j = upper_bound_u64(a.from, a.n_calls, q - 1);  // the calls with from < q
        if (j && q < a.to[j - 1]) {
            q = a.from[j - 1];
            ++snapped;
        }
    }
    u64 hb = 0;
    if (q <= b) {
        status = 13;
        info = b;
    } else {
        for (uint32_t c = threadIdx.x; c < a.n_classes; c += kBlock) a.ccur[c] = lower_bound_u32(a.cpos, a.ccur[c], a.cend[c], q);
        __syncthreads();
        hb = class_bound(a, sh);
    }
    if (threadIdx.x == 0u) {
        if (!status) a.bounds[g.s + 1] = q;
        g.out[0] = q;
        g.out[1] = status;
        g.out[2] = info;
        g.out[3] = probes;
        g.out[4] = snapped;
        g.out[5] = status ? 0 : g.PB[q - b];
        g.out[6] = status ? 0 : g.PM[q - b];
        g.out[7] = hb;
    }
}

struct EsCtx : Scratch {  // (its `extra`: the row lists of the handle under construction)
    time_index::Stage index{*this};
    Buf temp{*this}, small{*this}, key{*this}, pos{*this}, key_s{*this}, cpos{*this}, classes{*this}, bounds{*this}, first{*this}, heights{*this}, rows{*this}, offs{*this};
    Buf pos_of_row{*this}, acc{*this}, acc_s{*this}, astart{*this}, prefix{*this}, delta{*this}, table{*this}, head{*this};  // the meter's
    uint64_t stat_segments = 0, stat_classes = 0, stat_probes = 0, stat_snapped = 0;
    uint64_t meter_stats[6] = {0, 0, 0, 0, 0, 0};  // accesses, tiles, peak slots, nodes past the cuts, synchronisations, tables
    uint64_t meter_tile = 0;                       // the test knob: survives the calls
    void reset_stats() override {
        stat_segments = stat_classes = stat_probes = stat_snapped = 0;
        std::fill(meter_stats, meter_stats + 6, 0);
    }
};
thread_local EsCtx g_es;

size_t sort_class_temp(size_t n, unsigned bits) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_pairs(nullptr, bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint32_t*)nullptr, n, 0u, bits, stream());
    return std::max<size_t>(bytes, 16);
}

size_t sort_keys_temp(size_t n) {
    size_t bytes = 0;
    (void)rocprim::radix_sort_keys(nullptr, bytes, (u64*)nullptr, (u64*)nullptr, n, 0u, 64u, stream());
    return std::max<size_t>(bytes, 16);
}

// what the status-2 decision fixes of a metered cut
struct MeterPlan {
    u64 tile = 0, cap_b = 0, cap_m = 0, nodes = 0;  // positions per tile | B <= cap_b | M <= cap_m (the Poseidon2 bound folded in) | the most nodes a table holds
    size_t table_bytes = 0;
};

}  // namespace

}  // namespace pw

using namespace pw;

struct PwExecutionSegments {
    DeviceBuf lists;
    size_t n_airs = 0, n_apcs = 0, n_parts = 0;
    uint64_t S = 0, positions = 0, covered = 0, list_bytes = 0;
    std::vector<uint64_t> bounds, time_keys, first_call;  // [S + 1], [S], [S + 1]
    std::vector<uint32_t> pcs;                            // [S + 1]
    std::vector<uint32_t> heights;                        // [S x (n_airs + n_apcs)]
    std::vector<int64_t> part_of_air;                     // [n_airs], -1 = takes no part
    std::vector<uint32_t> rows;                           // [S x n_parts]
    std::vector<uint64_t> list_off;                       // [S x n_parts] in words
    std::vector<uint64_t> system_heights;                 // [S x 3] = B, M, 2 M of a metered cut (empty: not metered)
    uint32_t min_log_height = 0;
};

extern "C" void pw_execution_segments_destroy(PwExecutionSegments* e) { delete e; }

extern "C" void pw_execution_segments_sizes(const PwExecutionSegments* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->S;
    sizes[1] = e->n_airs;
    sizes[2] = e->n_apcs;
    sizes[3] = e->positions;
    sizes[4] = e->covered;
    sizes[5] = e->list_bytes;
}

extern "C" void pw_execution_segments_read_bounds(const PwExecutionSegments* e, uint64_t* positions, uint64_t* time_keys, uint32_t* pcs, uint64_t* first_call) {
    if (!e) return;
    if (positions) std::copy(e->bounds.begin(), e->bounds.end(), positions);
    if (time_keys) std::copy(e->time_keys.begin(), e->time_keys.end(), time_keys);
    if (pcs) std::copy(e->pcs.begin(), e->pcs.end(), pcs);
    if (first_call) std::copy(e->first_call.begin(), e->first_call.end(), first_call);
}

extern "C" void pw_execution_segments_read_heights(const PwExecutionSegments* e, uint64_t* rows) {
    if (!e || !rows) return;
    std::copy(e->heights.begin(), e->heights.end(), rows);
}

extern "C" int pw_execution_segments_rows(const PwExecutionSegments* e, uint32_t segment, uint32_t air, const uint32_t** d_idx, uint64_t* rows, uint32_t* log_height) {
    if (!e || segment >= e->S || air >= e->n_airs) return -1;
    if (d_idx) *d_idx = nullptr;
    if (rows) *rows = 0;
    if (log_height) *log_height = 0;
    const int64_t k = e->part_of_air[air];
    if (k < 0) return 0;
    const size_t at = (size_t)segment * e->n_parts + (size_t)k;
    const uint64_t n = e->rows[at];
    if (!n) return 0;
    const uint64_t h = padded_height(n, (uint64_t)1 << e->min_log_height);
    uint32_t lh = 0;
    while (((uint64_t)1 << lh) < h) ++lh;
    if (d_idx) *d_idx = (const uint32_t*)e->lists.p + e->list_off[at];
    if (rows) *rows = n;
    if (log_height) *log_height = lh;
    return 1;
}

extern "C" int pw_execution_segments_read_lists(const PwExecutionSegments* e, uint32_t* words, const uint32_t** d_base) {
    if (!e) return -1;
    if (d_base) *d_base = e->list_bytes ? (const uint32_t*)e->lists.p : nullptr;
    if (!words || !e->list_bytes) return 0;
    PW_HIP_TRY(hipMemcpyAsync(words, e->lists.p, e->list_bytes, hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

extern "C" void pw_execution_segments_read_system_heights(const PwExecutionSegments* e, uint64_t* rows) {
    if (!e || !rows) return;
    std::fill(rows, rows + 3 * e->S, 0);  // (a handle of the unmetered cut)
    std::copy(e->system_heights.begin(), e->system_heights.end(), rows);
}

extern "C" void pw_execution_segments_last_meter_stats(uint64_t* out) {
    if (out) std::copy(g_es.meter_stats, g_es.meter_stats + 6, out);
}

extern "C" void pw_execution_segments_set_meter_tile(uint64_t n) { g_es.meter_tile = n; }

extern "C" void pw_execution_segments_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_es.stat_segments;
    out[1] = g_es.stat_classes;
    out[2] = g_es.stat_probes;
    out[3] = g_es.stat_snapped;
    out[4] = g_es.peak();
    out[5] = g_es.held();
}

// the cut of both entry points: meter == NULL is pw_execution_segments_from_traces, every step of it as it was
static int execution_segments_cut(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, uint32_t final_pc,
                                  const uint32_t* cycle_counts, const uint32_t* apc_widths, size_t n_apcs, const uint32_t* call_apc_ids, const uint64_t* call_from,
                                  const uint64_t* call_to, size_t n_calls, const PwSegmentLimits* limits, const PwSystemMeter* meter, size_t scratch_bytes,
                                  PwExecutionSegments** out, uint32_t* status, uint64_t* info) {
    if (!out || !status || !info || !limits || bridge_bus >= bb::P || limits->max_log_height > 31u || limits->min_log_height > limits->max_log_height ||
        !time_index::one_segment(segment_of_air, n_airs) || !time_index::calls_well_formed(cycle_counts, n_apcs, call_apc_ids, call_from, call_to, n_calls))
        return -1;
    if (limits->max_cells && n_apcs && !apc_widths) return -1;
    for (size_t a = 0; a < n_apcs; ++a)
        if (limits->max_cells && !apc_widths[a]) return -1;
    time_index::Bridge B;
    if (!airs_well_formed(airs, n_airs) || !time_index::bridge_of(airs, n_airs, bridge_bus, &B) || B.M + 1 >= ((u64)1 << 32)) return -1;
    const u64 M = B.M, min_h = (u64)1 << limits->min_log_height, cap = (u64)1 << limits->max_log_height;
    const u64 max_segments = limits->max_segments ? limits->max_segments : kDefaultMaxSegments;
    // the meter: the interactions of the participating AIRs on the memory bus (no walk appends more accesses than acc_cap), the most of one row
    u64 acc_cap = 0, row_accesses = 0;
    if (meter) {
        if (meter->memory_bus >= bb::P || meter->tree_height < 1u || meter->tree_height > 30u) return -1;
        for (int k = 0; k < 3; ++k)
            if (meter->max_log_height[k] > 31u) return -1;
        bool seven_args = true;
        for (size_t a = 0; a < n_airs; ++a) {
            const u64 n = interactions_on(airs[a].prover, meter->memory_bus, kMemoryArgs, &seven_args);
            if (B.part_of_air[a] < 0) continue;
            acc_cap += n << airs[a].log_height;
            row_accesses = std::max(row_accesses, n);
        }
        if (!seven_args || acc_cap >= ((u64)1 << 32)) return -1;
    }
    EsCtx& cx = g_es;
    const ScratchCall call(cx, out, status, info);

    // ---- the AIRs that take part: those with the bridge; the calls per APC (host) ----
    const std::vector<size_t>& part_air = B.part_air;
    const std::vector<u64>& g0 = B.g0;
    const size_t n_parts = B.n_parts(), n_classes = n_parts + n_apcs;
    std::vector<u64> astart(n_apcs + 1, 0);  // the APC's first entry among the call starts grouped by APC
    u64 n_covered = 0;
    for (size_t j = 0; j < n_calls; ++j) {
        ++astart[call_apc_ids[j] + 1];
        n_covered += call_to[j] - call_from[j];
    }
    for (size_t a = 0; a < n_apcs; ++a) astart[a + 1] += astart[a];
    unsigned key_bits = 1;
    while (((u64)1 << key_bits) < 2 * (u64)n_parts) ++key_bits;

    // ---- status 2: what is known before a row is read ----
    const u64 seg_cap = std::min<u64>(max_segments, M);  // (a segment holds a position: S <= N <= M)
    MeterPlan mp;
    {
        // a list holds padded(rows) <= max(2^min_log_height, 2 * rows) words, rounded up to 4; the rows of all lists are the N positions
        const u64 n_lists = std::min<u64>(M, seg_cap * n_parts);
        const size_t list_bytes = (size_t)(2 * M + n_lists * std::max<u64>(min_h, 4)) * 4 + 16;
        const size_t tables = 4096 + n_calls * 24 + (n_apcs + 1) * 8 + n_classes * 40 + (n_parts + 2) * 32;
        const size_t per_segment = (size_t)(seg_cap + 1) * (8 + 12 + n_parts * 16) + std::min<size_t>(kHeightChunk + n_classes, (size_t)(seg_cap + 1) * n_classes) * 4;
        const size_t index_need = time_index::bytes_needed(M);
        const size_t class_need = 64 + (size_t)M * 32 + n_calls * 4 + (M ? sort_class_temp(M, key_bits) : 0);
        size_t need = ((size_t)1 << 20) + tables + std::max(index_need, class_need) + per_segment + list_bytes;
        if (meter) {
            // The node table holds the nodes of one segment's tiles: before the tile in which a system prefix passes its cap there
            // are at most min(cap_m, cap_b * levels) of them, the tile adds at most tile * (accesses of a row) * levels, and there
            // are never more than levels per access; twice as many slots as nodes (bus_shared.hpp's rule). Besides the table: the
            // position of every row (4 M), the accesses unsorted and sorted (16 each) with the sort's temporary storage, astart
            // (4 per position), the two prefix arrays (16 per position), the tile's deltas (8 per position of a tile), the head.
            mp.tile = std::min<u64>(cx.meter_tile ? cx.meter_tile : kDefaultMeterTile, std::max<u64>(M, 1));
            mp.cap_b = (u64)1 << meter->max_log_height[0];
            mp.cap_m = std::min<u64>((u64)1 << meter->max_log_height[1], ((u64)1 << meter->max_log_height[2]) >> 1);  // (2 M <= 2^c)
            const u64 levels = meter->tree_height + 1;
            mp.nodes = std::min<u64>(acc_cap * levels, std::min<u64>(mp.cap_m, mp.cap_b * levels) + mp.tile * row_accesses * levels);
            u64 slots = 1024;
            while (slots < 2 * mp.nodes) slots <<= 1;
            mp.table_bytes = (size_t)slots * kNodeSlotBytes;
            need += 4096 + sizeof(WalkHead) + (size_t)M * 4 + (size_t)acc_cap * 16 + (acc_cap ? sort_keys_temp(acc_cap) : 16) + (size_t)(M + 2) * 4 + (size_t)(M + 1) * 16 +
                    (size_t)mp.tile * 8 + mp.table_bytes;
        }
        if (call.bound(scratch_bytes) < need) {
            *status = 2;
            *info = need;
            return 0;
        }
    }

    auto result = std::make_unique<PwExecutionSegments>();
    PwExecutionSegments& R = *result;
    R.n_airs = n_airs;
    R.n_apcs = n_apcs;
    R.n_parts = n_parts;
    R.covered = n_covered;
    R.part_of_air = B.part_of_air;
    R.min_log_height = limits->min_log_height;
    cx.stat_classes = n_airs + n_apcs;

    // ---- index ----
    hipStream_t st = stream();
    u64 N = 0;
    PW_TRY(time_index::open(airs, segment_of_air, n_airs, bridge_bus, B, cx.index, cx.temp,
                            time_index::Names{"execution_segments_index_kernel", "execution_segments_sort_time", "execution_segments_time_kernel"}, &N, status, info));
    if (*status) return (int)hipGetLastError();
    cx.index.release_except({&cx.index.tkey_s, &cx.index.idx_s, &cx.index.pc_t});
    cx.temp.release();
    R.positions = N;
    if (!time_index::calls_within(call_to, n_calls, N, status, info)) return 0;
    R.bounds.assign(1, 0);
    R.pcs.assign(1, final_pc);
    R.first_call.assign(1, n_calls);
    if (!N) {  // nothing was executed (and so there is no call): no segment
        R.first_call[0] = 0;
        *out = result.release();
        return 0;
    }
    const dim3 block(kBlock);

    // ---- the meter's walk: the accesses (position << 32 | key) sorted, and the first access of every position ----
    u64 A = 0;
    if (meter) {
        u64 got[2] = {0, kEmpty};
        {
            ScopedKernelTimer timer("execution_meter_walk");
            PW_TRY(cx.head.ensure(sizeof(WalkHead)));
            PW_TRY(cx.pos_of_row.ensure(M * 4));
            PW_TRY(cx.acc.ensure(std::max<u64>(acc_cap, 1) * 8));
            u64* d_counters = cx.head.as<u64>();  // (the head's first words, until the tiles begin)
            PW_HIP_TRY(hipMemcpyAsync(d_counters, got, sizeof got, hipMemcpyHostToDevice, st));
            PW_HIP_TRY(hipMemsetAsync(cx.pos_of_row.p, 0xff, M * 4, st));
            hipLaunchKernelGGL(execution_meter_positions_kernel, dim3(div_up(N, kBlock)), block, 0, st, (const uint32_t*)cx.index.idx_s.p, N, cx.pos_of_row.as<uint32_t>());
            std::vector<Part> parts;
            if (acc_cap) PW_TRY(collect_parts(airs, n_airs, meter->memory_bus, parts, nullptr));
            for (const Part& part : parts) {
                const int64_t k = B.part_of_air[part.air];
                if (k < 0) continue;  // (not on the bridge: none of its rows is at a position)
                const Walked w = walked(airs[part.air]);
                with_fast(w.lp, [&](auto fast) {
                    hipLaunchKernelGGL(execution_meter_walk_kernel<decltype(fast)::value>, dim3(div_up(w.H, kBlock)), block, 0, st, part.vals, w.H, w.lp, w.order, part.begin,
                                       part.end, (uint32_t)part.air, g0[(size_t)k], (const uint32_t*)cx.pos_of_row.p, meter->tree_height, cx.acc.as<u64>(), acc_cap, d_counters);
                });
            }
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(got, d_counters, sizeof got, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
        }
        cx.pos_of_row.release();
        if (got[1] != kEmpty) {
            *status = 15;
            *info = got[1];
            return 0;
        }
        A = got[0];
        if (A > acc_cap) return (int)hipErrorInvalidValue;  // (cannot happen: more accesses than interactions)
        cx.meter_stats[0] = A;
        ScopedKernelTimer timer("execution_meter_sort");
        PW_TRY(cx.acc_s.ensure(std::max<u64>(A, 1) * 8));
        PW_TRY(cx.astart.ensure((N + 2) * 4));
        if (A)
            PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, cx.acc.as<u64>(), cx.acc_s.as<u64>(), (size_t)A, 0u, 64u, st); }));
        hipLaunchKernelGGL(execution_meter_starts_kernel, dim3(div_up(N + 1, kBlock)), block, 0, st, (const u64*)cx.acc_s.p, A, N, cx.astart.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipStreamSynchronize(st));
        cx.acc.release();
    }

    // ---- classify and sort: per class the ascending list of its positions ----
    char* sm = nullptr;
    size_t at_g0 = 0, at_from = 0, at_to = 0, at_astart = 0, at_width = 0, at_kstart = 0, at_cbeg = 0, at_cend = 0, at_ccur = 0, at_result = 0;
    {
        ScopedKernelTimer timer("execution_segments_classify");
        std::vector<u64> width(n_classes, 0);
        for (size_t k = 0; k < n_parts; ++k) width[k] = airs[part_air[k]].prover->width;
        for (size_t a = 0; a < n_apcs; ++a) width[n_parts + a] = apc_widths ? apc_widths[a] : 0;
        std::vector<uint32_t> afrom(n_calls, 0);  // the call starts grouped by APC, ascending inside an APC
        {
            std::vector<u64> next(astart.begin(), astart.end() - 1);
            for (size_t j = 0; j < n_calls; ++j) afrom[next[call_apc_ids[j]]++] = (uint32_t)call_from[j];
        }
        Image im;
        at_g0 = im.put(g0);
        at_from = im.put(std::vector<u64>(call_from, call_from + n_calls));
        at_to = im.put(std::vector<u64>(call_to, call_to + n_calls));
        at_astart = im.put(astart);
        at_width = im.put(width);
        at_kstart = im.put(std::vector<u64>(2 * n_parts + 1, 0));
        at_cbeg = im.put(std::vector<u64>(n_classes, 0));
        at_cend = im.put(std::vector<u64>(n_classes, 0));
        at_ccur = im.put(std::vector<u64>(n_classes, 0));
        at_result = im.put(std::vector<u64>(8, 0));
        PW_TRY(im.upload(cx.small, st));
        sm = cx.small.as<char>();
        PW_TRY(cx.key.ensure(N * 4));
        PW_TRY(cx.pos.ensure(N * 4));
        PW_TRY(cx.key_s.ensure(N * 4));
        PW_TRY(cx.cpos.ensure((N + n_calls) * 4 + 16));
        hipLaunchKernelGGL(execution_segments_classify_kernel, dim3(div_up(N, kBlock)), block, 0, st, (const uint32_t*)cx.index.idx_s.p, (const u64*)(sm + at_g0),
                           (uint32_t)n_parts, (const u64*)(sm + at_from), (const u64*)(sm + at_to), (uint32_t)n_calls, N, cx.key.as<uint32_t>(), cx.pos.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
        if (n_calls) PW_HIP_TRY(hipMemcpyAsync(cx.cpos.as<uint32_t>() + N, afrom.data(), n_calls * 4, hipMemcpyHostToDevice, st));
        PW_HIP_TRY(hipStreamSynchronize(st));  // (the image and afrom are locals)
    }
    {
        ScopedKernelTimer timer("execution_segments_sort_class");
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::radix_sort_pairs(t, b, cx.key.as<uint32_t>(), cx.key_s.as<uint32_t>(), cx.pos.as<uint32_t>(), cx.cpos.as<uint32_t>(), (size_t)N, 0u, key_bits, st);
        }));
        hipLaunchKernelGGL(execution_segments_starts_kernel, dim3(div_up(2 * n_parts + 1, 64)), dim3(64), 0, st, (const uint32_t*)cx.key_s.p, N, (uint32_t)(2 * n_parts),
                           (u64*)(sm + at_kstart));
        hipLaunchKernelGGL(execution_segments_classes_kernel, dim3(div_up(n_classes, 64)), dim3(64), 0, st, (const u64*)(sm + at_kstart), (const u64*)(sm + at_astart),
                           (uint32_t)n_parts, (uint32_t)n_apcs, N, (u64*)(sm + at_cbeg), (u64*)(sm + at_cend));
        PW_HIP_TRY(hipGetLastError());
    }

    // ---- the cuts ----
    const u64 bounds_cap = std::min<u64>(max_segments, N);
    u64 res[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    {
        ScopedKernelTimer timer(meter ? "execution_meter_cuts" : "execution_segments_bounds");
        PW_TRY(cx.bounds.ensure((bounds_cap + 1) * 8));
        BoundsArgs a{};
        a.cpos = (const uint32_t*)cx.cpos.p;
        a.cbeg = (const u64*)(sm + at_cbeg);
        a.cend = (const u64*)(sm + at_cend);
        a.cwidth = (const u64*)(sm + at_width);
        a.ccur = (u64*)(sm + at_ccur);
        a.from = (const u64*)(sm + at_from);
        a.to = (const u64*)(sm + at_to);
        a.bounds = cx.bounds.as<u64>();
        a.result = (u64*)(sm + at_result);
        a.N = N;
        a.cap = cap;
        a.min_h = min_h;
        a.max_cells = limits->max_cells;
        a.max_segments = max_segments;  // (after s cuts b >= s, so the loop writes at most min(max_segments, N) + 1 bounds)
        a.n_classes = (uint32_t)n_classes;
        a.n_calls = (uint32_t)n_calls;
        if (!meter) {
            hipLaunchKernelGGL(execution_segments_bounds_kernel, dim3(1), block, 0, st, a);
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(res, sm + at_result, sizeof res, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
        } else {
            // The segments one by one from the host: the tiles of a segment until a system prefix passes its cap or the class
            // height bound is reached (one synchronisation per tile, counted), then the one-workgroup step that sets b_(s+1).
            const u64 T = mp.tile;
            PW_TRY(cx.prefix.ensure((N + 1) * 16));
            PW_TRY(cx.delta.ensure(T * 8));
            u64 *PB = cx.prefix.as<u64>(), *PM = PB + (N + 1);
            uint32_t *dB = cx.delta.as<uint32_t>(), *dM = dB + T;
            PW_HIP_TRY(hipMemsetAsync(dB, 0, T * 8, st));
            WalkHead* d_head = cx.head.as<WalkHead>();
            const u64* d_acc = (const u64*)cx.acc_s.p;
            const uint32_t* d_astart = (const uint32_t*)cx.astart.p;
            u64* d_out = (u64*)(sm + at_result);
            uint64_t* ms = cx.meter_stats;
            u64 out8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            hipLaunchKernelGGL(execution_meter_open_kernel, dim3(1), block, 0, st, a, d_out);
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(out8, d_out, sizeof out8, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            ++ms[4];
            u64 b = 0, s = 0, hb = out8[7], first_slots = kStartSlots;
            while (b < N) {
                if (s == max_segments) {
                    res[1] = 14;
                    res[2] = b;
                    break;
                }
                NodeTable nt{};
                int walk_rc = 0;
                Grown g;
                WalkCounts wc;
                PW_TRY(grow_table(
                    cx.table, d_head, mp.nodes, kNodeSlotBytes, mp.table_bytes, first_slots, "execution_meter_clear",
                    [&](u64* tb, const TableRule& rule) {
                        const u64 slots = rule.mask + 1;
                        nt.v = TableView{rule, tb, nullptr};
                        nt.first = tb + slots;
                        ms[2] = std::max<uint64_t>(ms[2], slots);
                        ++ms[5];
                        return (int)hipMemsetAsync(tb, 0xff, slots * kNodeSlotBytes, st);
                    },
                    [&] {
                        ScopedKernelTimer tiles("execution_meter_tiles");
                        for (u64 lo = b; lo < hb && !walk_rc;) {
                            const u64 hi = std::min<u64>(lo + T, hb);
                            const dim3 grid(std::max(1u, div_up(std::min<u64>((hi - lo) * row_accesses, A), kBlock)));
                            hipLaunchKernelGGL(execution_meter_insert_kernel, grid, block, 0, st, d_acc, d_astart, lo, hi, meter->tree_height, nt, &d_head->c.overflow);
                            hipLaunchKernelGGL(execution_meter_count_kernel, grid, block, 0, st, d_acc, d_astart, lo, hi, meter->tree_height, nt,
                                               (const uint32_t*)&d_head->c.overflow, dB, dM);
                            hipLaunchKernelGGL(execution_meter_scan_kernel, dim3(1), block, 0, st, dB, dM, b, lo, hi, mp.cap_b, mp.cap_m, PB, PM, d_head->c.counts,
                                               (const uint32_t*)&d_head->c.overflow);
                            if ((walk_rc = (int)hipGetLastError()) != 0) break;
                            if ((walk_rc = (int)hipMemcpyAsync(&wc, d_head, sizeof wc, hipMemcpyDeviceToHost, st)) != 0) break;
                            if ((walk_rc = (int)hipStreamSynchronize(st)) != 0) break;
                            ++ms[1];
                            ++ms[4];
                            if (wc.overflow || wc.counts[2]) break;
                            lo = hi;
                        }
                    },
                    [] {}, &g));
                ++ms[4];  // (grow_table's own read-back)
                if (walk_rc) return walk_rc;
                if (g.no_table || g.overflowed()) return (int)hipErrorOutOfMemory;  // (cannot happen inside the bytes status 2 names)
                first_slots = g.slots;
                CloseArgs c{};
                c.a = a;
                c.PB = PB;
                c.PM = PM;
                c.b = b;
                c.s = s;
                c.q_max = g.c.counts[2] ? g.c.counts[2] - 1 : hb;
                for (int k = 0; k < 3; ++k) c.sys_width[k] = limits->max_cells ? meter->width[k] : 0;
                c.out = d_out;
                {
                    ScopedKernelTimer close("execution_meter_bounds");
                    hipLaunchKernelGGL(execution_meter_close_kernel, dim3(1), block, 0, st, c);
                    PW_HIP_TRY(hipGetLastError());
                    PW_HIP_TRY(hipMemcpyAsync(out8, d_out, sizeof out8, hipMemcpyDeviceToHost, st));
                    PW_HIP_TRY(hipStreamSynchronize(st));
                }
                ++ms[4];
                res[3] += out8[3];
                res[4] += out8[4];
                if (out8[1]) {
                    res[1] = out8[1];
                    res[2] = out8[2];
                    break;
                }
                R.system_heights.insert(R.system_heights.end(), {out8[5], out8[6], 2 * out8[6]});
                ms[3] += g.c.counts[1] - out8[6];
                b = out8[0];
                hb = out8[7];
                ++s;
            }
            res[0] = s;
        }
    }
    cx.table.release();
    cx.prefix.release();
    cx.delta.release();
    cx.acc_s.release();
    cx.astart.release();
    cx.head.release();
    cx.key.release();
    cx.pos.release();
    cx.temp.release();
    cx.stat_probes = res[3];
    cx.stat_snapped = res[4];
    if (res[1]) {
        *status = (uint32_t)res[1];
        *info = res[2];
        return 0;
    }
    const u64 S = res[0];
    R.S = S;
    cx.stat_segments = S;

    // ---- per segment: its bounds, first time key and pc, first call, class counts ----
    {
        ScopedKernelTimer timer("execution_segments_heights");
        R.bounds.resize(S + 1);
        R.time_keys.resize(S);
        R.pcs.assign(S + 1, final_pc);
        R.first_call.resize(S + 1);
        PW_TRY(cx.first.ensure(S * 8 + S * 4 + 16));
        u64* d_tk = cx.first.as<u64>();
        uint32_t* d_pc = (uint32_t*)(d_tk + S);
        hipLaunchKernelGGL(execution_segments_first_kernel, dim3(div_up(S, kBlock)), block, 0, st, (const u64*)cx.bounds.p, S, (const u64*)cx.index.tkey_s.p,
                           (const uint32_t*)cx.index.pc_t.p, d_tk, d_pc);
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipMemcpyAsync(R.bounds.data(), cx.bounds.p, (S + 1) * 8, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(R.time_keys.data(), d_tk, S * 8, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(R.pcs.data(), d_pc, S * 4, hipMemcpyDeviceToHost, st));
        R.heights.assign((size_t)S * (n_airs + n_apcs), 0);
        const u64 seg_chunk = std::max<u64>(1, kHeightChunk / n_classes);
        std::vector<uint32_t> h(std::min<u64>(seg_chunk, S) * n_classes);
        PW_TRY(cx.heights.ensure(h.size() * 4));
        for (u64 s0 = 0; s0 < S; s0 += seg_chunk) {
            const u64 s1 = std::min<u64>(S, s0 + seg_chunk), n = (s1 - s0) * n_classes;
            hipLaunchKernelGGL(execution_segments_heights_kernel, dim3(div_up(n, kBlock)), block, 0, st, (const uint32_t*)cx.cpos.p, (const u64*)(sm + at_cbeg),
                               (const u64*)(sm + at_cend), (uint32_t)n_classes, (const u64*)cx.bounds.p, s0, s1, cx.heights.as<uint32_t>());
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipMemcpyAsync(h.data(), cx.heights.p, n * 4, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            for (u64 s = s0; s < s1; ++s) {
                const uint32_t* src = h.data() + (s - s0) * n_classes;
                uint32_t* dst = R.heights.data() + (size_t)s * (n_airs + n_apcs);
                for (size_t k = 0; k < n_parts; ++k) dst[part_air[k]] = src[k];
                for (size_t a = 0; a < n_apcs; ++a) dst[n_airs + a] = src[n_parts + a];
            }
        }
        PW_HIP_TRY(hipStreamSynchronize(st));
        for (u64 s = 0; s <= S; ++s) R.first_call[s] = (u64)(std::lower_bound(call_from, call_from + n_calls, R.bounds[s]) - call_from);
        cx.first.release();
        cx.heights.release();
        cx.index.tkey_s.release();
        cx.index.pc_t.release();
    }

    // ---- the row lists ----
    {
        ScopedKernelTimer timer("execution_segments_lists");
        const size_t n_pairs = (size_t)S * n_parts;
        PW_TRY(cx.rows.ensure(n_pairs * 8));
        PW_TRY(cx.offs.ensure(n_pairs * 8));
        uint32_t* d_base = cx.rows.as<uint32_t>();
        uint32_t* d_rows = d_base + n_pairs;
        hipLaunchKernelGGL(execution_segments_rows_kernel, dim3(div_up(n_pairs, kBlock)), block, 0, st, (const uint32_t*)cx.cpos.p, (const u64*)(sm + at_kstart),
                           (uint32_t)n_parts, (const u64*)cx.bounds.p, S, d_base, d_rows);
        PW_HIP_TRY(hipGetLastError());
        R.rows.resize(n_pairs);
        R.list_off.assign(n_pairs, 0);
        PW_HIP_TRY(hipMemcpyAsync(R.rows.data(), d_rows, n_pairs * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        u64 words = 0;
        for (size_t i = 0; i < n_pairs; ++i) {
            R.list_off[i] = words;
            words += (padded_height(R.rows[i], min_h) + 3) & ~(u64)3;
        }
        R.list_bytes = words * 4;
        PW_TRY(R.lists.ensure(std::max<size_t>(words * 4, 16)));
        cx.set_extra(R.lists.bytes);
        PW_HIP_TRY(hipMemsetAsync(R.lists.p, 0xff, std::max<size_t>(words * 4, 16), st));
        PW_HIP_TRY(hipMemcpyAsync(cx.offs.p, R.list_off.data(), n_pairs * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(execution_segments_scatter_kernel, dim3(div_up(N, kBlock)), block, 0, st, (const uint32_t*)cx.key_s.p, (const uint32_t*)cx.cpos.p,
                           (const u64*)(sm + at_kstart), (const uint32_t*)cx.index.idx_s.p, (const u64*)(sm + at_g0), (uint32_t)n_parts, (const u64*)cx.bounds.p, S,
                           (const uint32_t*)d_base, (const u64*)cx.offs.p, N, (uint32_t*)R.lists.p);
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    *out = result.release();
    return 0;
}

extern "C" int pw_execution_segments_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, uint32_t final_pc,
                                                 const uint32_t* cycle_counts, const uint32_t* apc_widths, size_t n_apcs, const uint32_t* call_apc_ids,
                                                 const uint64_t* call_from, const uint64_t* call_to, size_t n_calls, const PwSegmentLimits* limits, size_t scratch_bytes,
                                                 PwExecutionSegments** out, uint32_t* status, uint64_t* info) {
    return execution_segments_cut(airs, segment_of_air, n_airs, bridge_bus, final_pc, cycle_counts, apc_widths, n_apcs, call_apc_ids, call_from, call_to, n_calls, limits, nullptr,
                                  scratch_bytes, out, status, info);
}

extern "C" int pw_execution_segments_from_traces_metered(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, uint32_t final_pc,
                                                         const uint32_t* cycle_counts, const uint32_t* apc_widths, size_t n_apcs, const uint32_t* call_apc_ids,
                                                         const uint64_t* call_from, const uint64_t* call_to, size_t n_calls, const PwSegmentLimits* limits,
                                                         const PwSystemMeter* meter, size_t scratch_bytes, PwExecutionSegments** out, uint32_t* status, uint64_t* info) {
    if (!meter) return -1;
    return execution_segments_cut(airs, segment_of_air, n_airs, bridge_bus, final_pc, cycle_counts, apc_widths, n_apcs, call_apc_ids, call_from, call_to, n_calls, limits, meter,
                                  scratch_bytes, out, status, info);
}
