// The sparse memory Merkle tree (include/powdr_prover.h pw_memory_tree_*): a binary Poseidon2 tree of height H over 2^H
// leaves of 8 words, kept on the device from segment to segment. Per level l = 0 .. H the STORED nodes: their sorted indices and
// digests (level 0: the payloads too); a subtree nobody has written hashes to Z_l and is not stored.
//   leaf digest = first 8 words of permute(payload | 0^8), node = first 8 words of permute(left | right): the tuple of BUS_COMPRESS.
//   update      validate_kernel, lookup_kernel (continuity + which keys are stored), merge_new_kernel / merge_old_kernel: the new
//               level 0 (both inputs sorted and unique: every output place is a rank, no order of arrival anywhere), then every
//               level above it from the level below: head_flag_kernel + a select give the first child of every parent,
//               level_kernel hashes one parent per lane; once a level has at most kTailNodes nodes one workgroup finishes the tree
//               (tail_kernel: the top of the tree is a chain of one or two nodes per level over most of its height).
//   records     the touched node sets T_0 = keys, T_l = unique(T_(l-1) >> 1) by the same flag + select (tail_kernel<false> for the
//               chain), records_kernel looks every touched node and its children up in the old tree (phase 0) and the new (phase 1).
//   incremental (pw_memory_tree_set_mode, opt-in) the levels above the threshold are rank merges too, the way level 0 is: found + a scan
//               rank T_l in the old level l, touched_parent_kernel hashes every node of T_l from its children in the new level l - 1,
//               move_kernel streams every other stored node to its new rank, unhashed; the tail and load mode are the rebuild's.
//   open        (pw_memory_tree_open; read-only) the multiproof of n keys in three launches whatever H is: open_flag_kernel,
//               one lane per (level, key), says which lanes own a node of T_l whose sibling is not in T_l; one scan ranks them;
//               open_gather_kernel looks the sibling up in its level and writes its digest (Z_l: not stored) at the rank, the level-0
//               lanes the payloads. No hashing, no tree buffers, nothing that depends on an order of arrival.
// The new tree is built into fresh buffers next to the old one and swapped in at the very end: any status or error leaves the tree
// as it was. The permutation is p2::permute with the parameters as a kernel argument (scalar loads, as the __constant__ copy of
// merkle.hip gives them).
#include "prover_state.hpp"
#include "scratch.hpp"

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <memory>
#include <vector>

namespace pw {

namespace {

typedef unsigned long long u64;
constexpr int kBlock = 256;
constexpr int kMaxHeight = 40;
constexpr u64 kNoIndex = ~0ull;

struct LevelView { const u64* idx; const uint32_t* dig; u64 n; };
struct Digest { uint32_t w[8]; };

}  // namespace

// a level with at most this many nodes is finished, with everything above it, by one workgroup of as many threads
constexpr size_t kMemoryTreeTailNodes = 1024;

}  // namespace pw

struct PwMemoryTree {
    uint32_t height = 0;
    uint32_t ext_rc[8][16], int_rc[13];  // the table the tree was created under (Montgomery words)
    uint32_t zero[pw::kMaxHeight + 1][8];    // Z_0 .. Z_H (Montgomery)
    int device = -1;                     // the device its buffers live on, once it has any
    pw::DeviceBuf zbuf;                  // Z_0 .. Z_H on the device
    struct Data {
        std::vector<pw::LevelView> lv;   // H + 1 views into bufs
        const uint32_t* payload = nullptr;
        std::vector<std::unique_ptr<pw::DeviceBuf>> bufs;
        uint64_t nodes = 0;
        size_t bytes = 0;
        uint32_t root[8];
    } data;
    uint64_t last_permutations = 0, last_launches = 0, last_scratch = 0;
    uint32_t mode = PW_MEMORY_TREE_REBUILD;
};

namespace pw {

namespace {

constexpr size_t kTail = kMemoryTreeTailNodes;

__device__ __forceinline__ u64 lower_bound(const u64* __restrict__ a, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ void load8(const uint32_t* p, uint32_t* w) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
__device__ __forceinline__ void store8(uint32_t* p, const uint32_t* w) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// err[0] = the first key that is not above its predecessor or not below 2^H, err[1] = the first key with a payload word >= p
__global__ __launch_bounds__(kBlock) void validate_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ init, const uint32_t* __restrict__ fin,
                                                           u64 n, uint32_t H, u64* __restrict__ err) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const u64 k = keys[i];
    if ((k >> H) != 0 || (i > 0 && keys[i - 1] >= k)) atomicMin(err, i);
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 8; ++j) bad |= fin[i * 8 + j] >= bb::P || (init && init[i * 8 + j] >= bb::P);
    if (bad) atomicMin(err + 1, i);
}

// found[i] = key i is a stored leaf; with `init`: err[2] = the smallest key whose stored payload (zero: not stored) is not init
__global__ __launch_bounds__(kBlock) void lookup_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ init, u64 n, LevelView old,
                                                         const uint32_t* __restrict__ payload, u64* __restrict__ found, u64* __restrict__ err) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) { found[n] = 0; return; }  // (the scan's last place: the total)
    const u64 k = keys[i];
    const u64 at = lower_bound(old.idx, old.n, k);
    const bool have = at < old.n && old.idx[at] == k;
    found[i] = have ? 1ull : 0ull;
    if (!init) return;
    bool same = true;
#pragma unroll
    for (int j = 0; j < 8; ++j) same &= init[i * 8 + j] == (have ? payload[at * 8 + j] : 0u);
    if (!same) atomicMin(err + 2, k);
}

// The merged level 0: key j of the update lands behind the stored keys below it and the update's keys below it, the ones that are
// both counted once (before[j] = how many of the update's keys below j are stored); a stored key that the update does not name keeps
// its payload and digest.
__global__ __launch_bounds__(kBlock) void merge_new_kernel(const u64* __restrict__ keys, const uint32_t* __restrict__ fin, u64 n, LevelView old,
                                                            const u64* __restrict__ before, const p2::Params P, u64* __restrict__ idx,
                                                            uint32_t* __restrict__ payload, uint32_t* __restrict__ dig) {
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (j >= n) return;
    const u64 k = keys[j];
    const u64 at = j + lower_bound(old.idx, old.n, k) - before[j];
    uint32_t st[16];
    load8(fin + j * 8, st);
#pragma unroll
    for (int i = 8; i < 16; ++i) st[i] = 0u;
    idx[at] = k;
    store8(payload + at * 8, st);
    p2::permute(st, P);
    store8(dig + at * 8, st);
}

__global__ __launch_bounds__(kBlock) void merge_old_kernel(const u64* __restrict__ keys, u64 n, LevelView old, const uint32_t* __restrict__ old_payload,
                                                            const u64* __restrict__ before, u64* __restrict__ idx, uint32_t* __restrict__ payload,
                                                            uint32_t* __restrict__ dig) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= old.n) return;
    const u64 k = old.idx[i];
    const u64 c = lower_bound(keys, n, k);
    if (c < n && keys[c] == k) return;  // rewritten by the update
    const u64 at = i + c - before[c];
    uint32_t w[8];
    idx[at] = k;
    load8(old_payload + i * 8, w);
    store8(payload + at * 8, w);
    load8(old.dig + i * 8, w);
    store8(dig + at * 8, w);
}

// flags[i] = node i is the first stored child of its parent
__global__ __launch_bounds__(kBlock) void head_flag_kernel(const u64* __restrict__ idx, u64 n, uint8_t* __restrict__ flags) {
    const u64 i = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    flags[i] = (i == 0 || (idx[i] >> 1) != (idx[i - 1] >> 1)) ? 1 : 0;
}

__global__ __launch_bounds__(kBlock) void gather_parent_kernel(const u64* __restrict__ idx, const u64* __restrict__ head, u64 n_parents, u64* __restrict__ out) {
    const u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (p < n_parents) out[p] = idx[head[p]] >> 1;
}

// One level: parent p = compress(left, right) of its one or two adjacent stored children, `z` (the digest of an unwritten subtree of
// the children's level) for the missing side. One lane per parent, the digests as two 16-byte loads and stores each (compress_kernel).
__global__ __launch_bounds__(kBlock) void level_kernel(const u64* __restrict__ cidx, const uint32_t* __restrict__ cdig, u64 n_children,
                                                        const u64* __restrict__ head, u64 n_parents, const Digest z, const p2::Params P,
                                                        u64* __restrict__ pidx, uint32_t* __restrict__ pdig) {
    const u64 p = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (p >= n_parents) return;
    const u64 i = head[p];
    const u64 a = cidx[i];
    uint32_t st[16];
    if (a & 1ull) {
#pragma unroll
        for (int k = 0; k < 8; ++k) st[k] = z.w[k];
        load8(cdig + i * 8, st + 8);
    } else {
        load8(cdig + i * 8, st);
        if (i + 1 < n_children && cidx[i + 1] == a + 1) {
            load8(cdig + (i + 1) * 8, st + 8);
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) st[8 + k] = z.w[k];
        }
    }
    p2::permute(st, P);
    pidx[p] = a >> 1;
    store8(pdig + p * 8, st);
}

// Incremental mode, level l >= 1: the new level is the rank merge of the old level with the touched set T_l (sorted, unique), as level 0
// is of the stored keys with the update's. Touched node j lands behind the old nodes below it and the touched nodes below it, the ones
// that are both counted once (before[j] = how many of the touched nodes below j are stored in the old level), and is hashed from its
// one or two children in the NEW level below: one lower_bound for 2t, the sibling adjacent, `z` for a missing side. A touched node has a
// touched child, and every touched node of the level below is stored in the new tree: at least one side is found.
__global__ __launch_bounds__(kBlock) void touched_parent_kernel(const u64* __restrict__ t, u64 m, const u64* __restrict__ before, LevelView old, LevelView ch,
                                                                 const Digest z, const p2::Params P, u64* __restrict__ pidx, uint32_t* __restrict__ pdig) {
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (j >= m) return;
    const u64 node = t[j];
    const u64 at = j + lower_bound(old.idx, old.n, node) - before[j];
    u64 c = lower_bound(ch.idx, ch.n, 2 * node);
    uint32_t st[16];
    if (c < ch.n && ch.idx[c] == 2 * node) {
        load8(ch.dig + c * 8, st);
        ++c;
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) st[k] = z.w[k];
    }
    if (c < ch.n && ch.idx[c] == 2 * node + 1) {
        load8(ch.dig + c * 8, st + 8);
    } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) st[8 + k] = z.w[k];
    }
    p2::permute(st, P);
    pidx[at] = node;
    store8(pdig + at * 8, st);
}

// The old nodes of that level that are not in T_l move to their new rank with index and digest, unhashed: 40 bytes per node. Two lanes
// per node, each one 16-byte half of the digest, so a wave reads and writes runs of contiguous 16-byte words (the ranks of neighbours
// differ only where a new node lands between them); the first lane of a pair moves the 8-byte index. The rank needs the node's place
// in T_l: the workgroup's first and last nodes bound it (the same two searches in every lane), and between two touched nodes that
// leaves nothing to search.
constexpr int kMoveNodes = kBlock / 2;
__global__ __launch_bounds__(kBlock) void move_kernel(LevelView old, const u64* __restrict__ t, u64 m, const u64* __restrict__ before, u64* __restrict__ idx,
                                                       uint32_t* __restrict__ dig) {
    const u64 first = (u64)blockIdx.x * kMoveNodes;
    const u64 i = first + (threadIdx.x >> 1);
    if (i >= old.n) return;
    const u64 last = first + kMoveNodes <= old.n ? first + kMoveNodes - 1 : old.n - 1;
    const u64 lo = lower_bound(t, m, old.idx[first]);
    const u64 hi = lower_bound(t + lo, m - lo, old.idx[last]);  // the touched nodes below the last node, counted from lo
    const u64 node = old.idx[i];
    const u64 c = lo + lower_bound(t + lo, hi, node);
    if (c < m && t[c] == node) return;  // hashed again by touched_parent_kernel
    const u64 at = i + c - before[c];
    const unsigned half = threadIdx.x & 1u;
    reinterpret_cast<uint4*>(dig)[at * 2 + half] = reinterpret_cast<const uint4*>(old.dig)[i * 2 + half];
    if (!half) idx[at] = node;
}

// The levels first .. last from the level below `first` (n0 <= kTail nodes), in one workgroup of kTail threads: thread i owns child
// i, the heads are ranked by ballots and a prefix over the waves' totals, level l goes to slot l - first of idx_out / dig_out (kTail
// nodes each) and its size to counts[l - first]. A level written by the workgroup is made visible to its other waves by
// __threadfence_block() + the barrier (compress_tail_kernel). HASH = false: indices only (the touched node sets).
struct TailArgs {
    const u64* idx0; const uint32_t* dig0; u64 n0;
    int first, last;
    u64* idx_out; uint32_t* dig_out; u64* counts;
    const uint32_t* zero;  // 8 words per level (HASH)
};
template <bool HASH>
__global__ __launch_bounds__(kTail) void tail_kernel(const TailArgs a, const p2::Params P) {
    __shared__ uint32_t wave_total[kTail / 64];
    const u64* idx = a.idx0;
    const uint32_t* dig = a.dig0;
    u64 n = a.n0;
    const unsigned i = threadIdx.x, lane = i & 63u, wave = i >> 6;
    for (int l = a.first; l <= a.last; ++l) {
        u64* oi = a.idx_out + (size_t)(l - a.first) * kTail;
        uint32_t* od = HASH ? a.dig_out + (size_t)(l - a.first) * kTail * 8 : nullptr;
        u64 me = 0;
        bool head = false;
        if (i < n) {
            me = idx[i];
            head = i == 0 || (idx[i - 1] >> 1) != (me >> 1);
        }
        const u64 heads = __builtin_amdgcn_ballot_w64(head);
        if (lane == 0) wave_total[wave] = (uint32_t)__builtin_popcountll(heads);
        __syncthreads();
        uint32_t base = 0, total = 0;
        for (unsigned w = 0; w < kTail / 64; ++w) {
            if (w < wave) base += wave_total[w];
            total += wave_total[w];
        }
        if (head) {
            const uint32_t at = base + (uint32_t)__builtin_popcountll(heads & ((1ull << lane) - 1ull));
            oi[at] = me >> 1;
            if (HASH) {
                const uint32_t* z = a.zero + (size_t)(l - 1) * 8;
                uint32_t st[16];
                if (me & 1ull) {
                    load8(z, st);
                    load8(dig + (size_t)i * 8, st + 8);
                } else {
                    load8(dig + (size_t)i * 8, st);
                    if (i + 1 < n && idx[i + 1] == me + 1) load8(dig + (size_t)(i + 1) * 8, st + 8);
                    else load8(z, st + 8);
                }
                p2::permute(st, P);
                store8(od + (size_t)at * 8, st);
            }
        }
        if (i == 0) a.counts[l - a.first] = total;
        __threadfence_block();
        __syncthreads();
        idx = oi;
        dig = od;
        n = total;
    }
}

// The record rows of the levels first .. first + gridDim.y - 1, both phases (blockIdx.z): row = phase * phase_rows + lv[l].row + j for
// the j-th touched node of level l, looked up with its children in tree[phase]; what is not stored is the default of its level.
struct RecLevel { const u64* t; u64 n; u64 row; };
struct RecArgs {
    LevelView tree[2][kMaxHeight + 1];
    const uint32_t* payload[2];
    RecLevel lv[kMaxHeight + 1];
    int first;
    u64 phase_rows, pitch;
    uint32_t* rec;
    u64* ids;
    const uint32_t* zero;
};
__global__ __launch_bounds__(kBlock) void records_kernel(const RecArgs a) {
    const int l = a.first + (int)blockIdx.y;
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (j >= a.lv[l].n) return;
    const unsigned ph = blockIdx.z;
    const u64 t = a.lv[l].t[j];
    const u64 row = (u64)ph * a.phase_rows + a.lv[l].row + j;
    uint32_t w[24];
    const LevelView me = a.tree[ph][l];
    const u64 at = lower_bound(me.idx, me.n, t);
    const bool have = at < me.n && me.idx[at] == t;
    if (have) load8(me.dig + at * 8, w + 16); else load8(a.zero + (size_t)l * 8, w + 16);
    if (l == 0) {
        if (have) load8(a.payload[ph] + at * 8, w);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = 0u;
        }
#pragma unroll
        for (int k = 8; k < 16; ++k) w[k] = 0u;
    } else {
        const LevelView ch = a.tree[ph][l - 1];
        const uint32_t* z = a.zero + (size_t)(l - 1) * 8;
        u64 c = lower_bound(ch.idx, ch.n, 2 * t);
        if (c < ch.n && ch.idx[c] == 2 * t) { load8(ch.dig + c * 8, w); ++c; } else load8(z, w);
        if (c < ch.n && ch.idx[c] == 2 * t + 1) load8(ch.dig + c * 8, w + 8); else load8(z, w + 8);
    }
    uint32_t* out = a.rec + row;
    out[0] = bb::R_MOD_P;  // valid = 1
#pragma unroll
    for (int k = 0; k < 24; ++k) out[(size_t)(1 + k) * a.pitch] = w[k];
    if (a.ids) a.ids[row] = ((u64)ph << 63) | ((u64)l << 56) | t;
}

// ---- the multi-opening (pw_memory_tree_open) ------------------------------------------------------------------------------------------
// Lane (l, j) = (blockIdx.y, blockIdx.x * kBlock + threadIdx.x) stands for the node t = key_j >> l of T_l and owns it when key_(j-1)
// is not below it too. Its sibling t ^ 1 is in T_l iff, t odd: key_(j-1) >> l == t - 1 (the keys are sorted: the key before the first
// one below t); t even: the first key at or past (t + 1) << l — searched among the keys behind j only — is below t + 2 as well.
// flags[l * n + j] = the lane owns a node whose sibling the proof has to carry. The level-0 lanes apply validate_kernel's rule to the
// keys on the way (err[0]); with malformed keys the flags mean nothing, and every read stays inside keys[0 .. n).
__global__ __launch_bounds__(kBlock) void open_flag_kernel(const u64* __restrict__ keys, u64 n, uint32_t H, uint8_t* __restrict__ flags, u64* __restrict__ err) {
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t l = blockIdx.y;
    if (j == 0 && l == 0) flags[n * H] = 0;  // (the scan's last place: the total)
    if (j >= n) return;
    const u64 k = keys[j];
    const u64 before = j > 0 ? keys[j - 1] : 0;
    if (l == 0 && ((k >> H) != 0 || (j > 0 && before >= k))) atomicMin(err, j);
    const u64 t = k >> l;
    bool carry = j == 0 || (before >> l) != t;
    if (carry) {
        if (t & 1ull) {
            carry = j == 0 || (before >> l) != t - 1;
        } else {
            // the keys below t end a run that starts at j: short on the low levels, where most lanes own a node — gallop, then search
            const u64 first = (t + 1) << l;
            u64 lo = j + 1, hi = j + 1;
            for (u64 step = 1; hi < n && keys[hi] < first; step <<= 1) { lo = hi + 1; hi += step; }
            hi = hi < n ? hi : n;
            const u64 c = lo + lower_bound(keys + lo, hi - lo, first);
            carry = c >= n || (keys[c] >> l) != t + 1;
        }
    }
    flags[(u64)l * n + j] = carry ? 1 : 0;
}

// The flagged lanes: one lower_bound for t ^ 1 in level l's sorted indices, the digest (Z_l where it is not stored) as two 16-byte
// loads and two 16-byte stores at the lane's rank. The level-0 lanes look their key up as well and write its payload row.
struct FlagToCount {
    __host__ __device__ u64 operator()(uint8_t f) const { return f; }
};
struct OpenArgs {
    LevelView lv[kMaxHeight];  // levels 0 .. H - 1: the root has no sibling
    const uint32_t* payload;
    const uint32_t* zero;
};
__global__ __launch_bounds__(kBlock) void open_gather_kernel(const OpenArgs a, const u64* __restrict__ keys, u64 n, const uint8_t* __restrict__ flags,
                                                              const u64* __restrict__ rank, uint32_t* __restrict__ payloads, uint32_t* __restrict__ siblings) {
    const u64 j = (u64)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t l = blockIdx.y;
    if (j >= n) return;
    const u64 i = (u64)l * n + j;
    const bool carry = flags[i] != 0;
    if (!carry && l != 0) return;
    const u64 k = keys[j];
    const LevelView me = a.lv[l];
    uint32_t w[8];
    if (l == 0) {
        const u64 at = lower_bound(me.idx, me.n, k);
        if (at < me.n && me.idx[at] == k) load8(a.payload + at * 8, w);
        else {
#pragma unroll
            for (int q = 0; q < 8; ++q) w[q] = 0u;
        }
        store8(payloads + j * 8, w);
        if (!carry) return;
    }
    const u64 s = (k >> l) ^ 1ull;
    const u64 at = lower_bound(me.idx, me.n, s);
    if (at < me.n && me.idx[at] == s) load8(me.dig + at * 8, w); else load8(a.zero + (size_t)l * 8, w);
    store8(siblings + rank[i] * 8, w);
}

// One lane per row of the memory boundary AIR's trace. THE COLUMN POSITIONS ARE THOSE OF BOUNDARY_COLUMNS (powdr_amd/system_airs.py;
// system_traces.hip boundary_rows_kernel writes them): [is_valid, as, ptr, p_lo, p_hi, init0..3, init_ts, fin0..3, fin_ts, ...] — the
// two must move together.
constexpr uint32_t kColAs = 1, kColPtr = 2, kColInit = 5, kColFin = 10;
__global__ __launch_bounds__(kBlock) void boundary_leaves_kernel(const uint32_t* __restrict__ trace, u64 pitch, u64 n, u64* __restrict__ keys,
                                                                  uint32_t* __restrict__ init, uint32_t* __restrict__ fin) {
    const u64 r = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (r >= n) return;
    const u64 as = bb::from_monty(trace[kColAs * pitch + r]), ptr = bb::from_monty(trace[kColPtr * pitch + r]);
    keys[r] = ((as - 1) << 29) + ptr;
    uint32_t a[8], b[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        a[k] = k < 4 ? trace[(kColInit + k) * pitch + r] : 0u;
        b[k] = k < 4 ? trace[(kColFin + k) * pitch + r] : 0u;
    }
    store8(init + r * 8, a);
    store8(fin + r * 8, b);
}

// ---- host --------------------------------------------------------------------------------------------------------------------------
struct TreeCtx : Scratch {
    DeviceBuf small;  // errors | a count | the tail's level sizes: stays and is not accounted (a few hundred bytes)
    Buf found{*this}, before{*this}, flags{*this}, head{*this}, ping{*this}, pong{*this}, temp{*this}, tail_t{*this};
    // incremental mode: the touched sets above the tail's stay until the levels are merged (tset[l] = T_l, wherever it lives); as
    // many buffers as the call has levels, so they are counted as the scratch's `extra`
    std::vector<std::unique_ptr<DeviceBuf>> kept;
    std::vector<const u64*> tset;
    uint64_t launches = 0;
    size_t kept_bytes() const {
        size_t b = 0;
        for (const auto& k : kept) b += k->bytes;
        return b;
    }
    void release() override {
        Scratch::release();
        kept.clear();
        tset.clear();
    }
    void reset_stats() override { launches = 0; }
};
thread_local TreeCtx g_tree;
constexpr size_t kErr = 0, kCount = 4, kTailCounts = 8;  // u64 places in TreeCtx::small
constexpr size_t kSmallWords = kTailCounts + kMaxHeight + 1;

bool same_table(const PwMemoryTree* t) {
    const p2::Params& p = poseidon2_params_host();
    return memcmp(t->ext_rc, p.ext_rc, sizeof t->ext_rc) == 0 && memcmp(t->int_rc, p.int_rc, sizeof t->int_rc) == 0;
}

// head[0 .. *count) = the positions of the first stored child of every parent of the level idx[0 .. n); with `count`: read back
int select_heads(TreeCtx& cx, const u64* idx, u64 n, u64* count) {
    hipStream_t st = stream();
    PW_HIP_TRY((hipError_t)cx.flags.ensure(n));
    PW_HIP_TRY((hipError_t)cx.head.ensure(n * 8));
    hipLaunchKernelGGL(head_flag_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, st, idx, n, cx.flags.as<uint8_t>());
    u64* d_count = cx.small.as<u64>() + kCount;
    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
        return rocprim::select(t, b, rocprim::counting_iterator<u64>(0), cx.flags.as<uint8_t>(), cx.head.as<u64>(), d_count, (size_t)n, st);
    }));
    cx.launches += 2;
    if (count) {
        PW_HIP_TRY(hipMemcpyAsync(count, d_count, 8, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    }
    return 0;
}

// The touched node sets T_0 = keys, T_l = unique(T_(l-1) >> 1). rec == nullptr: their sizes into sizes[0 .. H]. Otherwise the sizes are
// given and every level's record rows are written as soon as its set exists (rec->lv[l].row set by the caller). keep (with the sizes
// pass): every set stays, in a buffer of its own or in the tail's slots, and cx.tset[l] says where; a records pass that finds them
// there only writes the rows.
int touched_levels(TreeCtx& cx, const PwMemoryTree* tree, const u64* d_keys, u64 n, std::vector<u64>& sizes, RecArgs* rec, bool keep = false) {
    hipStream_t st = stream();
    const int H = (int)tree->height;
    const p2::Params& P = poseidon2_params_host();
    auto emit = [&](int first, int levels, u64 widest) {
        rec->first = first;
        hipLaunchKernelGGL(records_kernel, dim3(div_up(widest, kBlock), levels, 2), dim3(kBlock), 0, st, *rec);
        ++cx.launches;
    };
    if (!rec) sizes.assign(H + 1, 0);
    sizes[0] = n;
    if (rec) {
        rec->lv[0].t = d_keys; rec->lv[0].n = n;
        emit(0, 1, n);
    }
    const u64* cur = d_keys;
    int l = 1;
    if (rec && !cx.tset.empty()) {  // the sets of the sizes pass are still there
        for (; l <= H && sizes[l - 1] > kTail; ++l) {
            rec->lv[l].t = cx.tset[l]; rec->lv[l].n = sizes[l];
            emit(l, 1, sizes[l]);
        }
        if (l <= H) {
            u64 widest = 0;
            for (int k = l; k <= H; ++k) {
                rec->lv[k].t = cx.tset[k]; rec->lv[k].n = sizes[k];
                widest = std::max(widest, sizes[k]);
            }
            emit(l, H - l + 1, widest);
        }
        return (int)hipGetLastError();
    }
    if (keep) {
        cx.tset.assign(H + 1, nullptr);
        cx.tset[0] = d_keys;
    }
    for (; l <= H && sizes[l - 1] > kTail; ++l) {
        const u64 m = sizes[l - 1];
        PW_TRY(select_heads(cx, cur, m, rec ? nullptr : &sizes[l]));
        if (keep) cx.kept.emplace_back(new DeviceBuf);
        DeviceBuf& out = keep ? *cx.kept.back() : (l & 1) ? cx.ping : cx.pong;
        PW_HIP_TRY((hipError_t)out.ensure(keep ? sizes[l] * 8 : m * 8));
        cx.set_extra(cx.kept_bytes());  // (and notes the peak, whichever buffer `out` is)
        hipLaunchKernelGGL(gather_parent_kernel, dim3(div_up(sizes[l], kBlock)), dim3(kBlock), 0, st, cur, cx.head.as<u64>(), sizes[l], out.as<u64>());
        ++cx.launches;
        cur = out.as<u64>();
        if (keep) cx.tset[l] = cur;
        if (rec) {
            rec->lv[l].t = cur; rec->lv[l].n = sizes[l];
            emit(l, 1, sizes[l]);
        }
    }
    if (l <= H) {
        const int levels = H - l + 1;
        PW_HIP_TRY((hipError_t)cx.tail_t.ensure((size_t)levels * kTail * 8));
        u64* d_counts = cx.small.as<u64>() + kTailCounts;
        const TailArgs a{cur, nullptr, sizes[l - 1], l, H, cx.tail_t.as<u64>(), nullptr, d_counts, nullptr};
        hipLaunchKernelGGL(tail_kernel<false>, dim3(1), dim3(kTail), 0, st, a, P);
        ++cx.launches;
        if (!rec) {
            PW_HIP_TRY(hipMemcpyAsync(&sizes[l], d_counts, (size_t)levels * 8, hipMemcpyDeviceToHost, st));
            PW_HIP_TRY(hipStreamSynchronize(st));
            if (keep)
                for (int k = l; k <= H; ++k) cx.tset[k] = cx.tail_t.as<u64>() + (size_t)(k - l) * kTail;
        } else {
            u64 widest = 0;
            for (int k = l; k <= H; ++k) {
                rec->lv[k].t = cx.tail_t.as<u64>() + (size_t)(k - l) * kTail; rec->lv[k].n = sizes[k];
                widest = std::max(widest, sizes[k]);
            }
            emit(l, levels, widest);
        }
    }
    return (int)hipGetLastError();
}

// One level of the incremental mode: the rank merge of the old level l with T_l (cx.tset[l], m nodes) into a fresh buffer. found +
// scan as for level 0, then ONE read-back — how many of T_l the old level stores, which gives the new level's size — counted among the
// launches: it is the dependent step of the level.
int merge_level(TreeCtx& cx, PwMemoryTree* tree, const PwMemoryTree::Data& old, PwMemoryTree::Data& d, int l, u64 m) {
    hipStream_t st = stream();
    const p2::Params& P = poseidon2_params_host();
    const LevelView o = old.lv[l], c = d.lv[l - 1];
    const u64* t = cx.tset[l];
    hipLaunchKernelGGL(lookup_kernel, dim3(div_up(m + 1, kBlock)), dim3(kBlock), 0, st, t, (const uint32_t*)nullptr, m, o, (const uint32_t*)nullptr, cx.found.as<u64>(),
                       cx.small.as<u64>() + kErr);
    PW_TRY(with_temp(cx.temp, [&](void* tmp, size_t& b) {
        return rocprim::exclusive_scan(tmp, b, cx.found.as<u64>(), cx.before.as<u64>(), 0ull, m + 1, rocprim::plus<u64>(), st);
    }));
    u64 n_found = 0;
    PW_HIP_TRY(hipMemcpyAsync(&n_found, cx.before.as<u64>() + m, 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    cx.launches += 3;
    if (n_found > m || n_found > o.n) return -1;
    const u64 parents = o.n + m - n_found;
    d.bufs.emplace_back(new DeviceBuf);
    DeviceBuf& b = *d.bufs.back();
    PW_HIP_TRY((hipError_t)b.ensure((size_t)parents * 40));
    uint32_t* dig = b.as<uint32_t>();
    u64* idx = reinterpret_cast<u64*>(dig + (size_t)parents * 8);
    Digest z;
    memcpy(z.w, tree->zero[l - 1], sizeof z.w);
    {
        ScopedKernelTimer tm("memory_tree_touched_kernel");
        hipLaunchKernelGGL(touched_parent_kernel, dim3(div_up(m, kBlock)), dim3(kBlock), 0, st, t, m, cx.before.as<u64>(), o, c, z, P, idx, dig);
    }
    ++cx.launches;
    if (o.n) {
        ScopedKernelTimer tm("memory_tree_move_kernel");
        hipLaunchKernelGGL(move_kernel, dim3(div_up(o.n, kMoveNodes)), dim3(kBlock), 0, st, o, t, m, cx.before.as<u64>(), idx, dig);
        ++cx.launches;
    }
    d.lv[l] = LevelView{idx, dig, parents};
    return 0;
}

// The tree over the merged level 0 (already in `d`): every level above it, the root read back. sizes != nullptr (incremental mode; the
// touched sets in cx.tset): the levels above the threshold are merged from `old`, only |T_l| nodes of each hashed.
int build_levels(TreeCtx& cx, PwMemoryTree* tree, const PwMemoryTree::Data& old, PwMemoryTree::Data& d, const std::vector<u64>* sizes, uint64_t* permutations) {
    hipStream_t st = stream();
    const int H = (int)tree->height;
    const p2::Params& P = poseidon2_params_host();
    int l = 1;
    for (; l <= H && d.lv[l - 1].n > kTail; ++l) {
        if (sizes) {
            PW_TRY(merge_level(cx, tree, old, d, l, (*sizes)[l]));
            *permutations += (*sizes)[l];
            continue;
        }
        const LevelView c = d.lv[l - 1];
        u64 parents = 0;
        PW_TRY(select_heads(cx, c.idx, c.n, &parents));
        d.bufs.emplace_back(new DeviceBuf);
        DeviceBuf& b = *d.bufs.back();
        PW_HIP_TRY((hipError_t)b.ensure((size_t)parents * 40));
        uint32_t* dig = b.as<uint32_t>();
        u64* idx = reinterpret_cast<u64*>(dig + (size_t)parents * 8);
        Digest z;
        memcpy(z.w, tree->zero[l - 1], sizeof z.w);
        ScopedKernelTimer t("memory_tree_level_kernel");
        hipLaunchKernelGGL(level_kernel, dim3(div_up(parents, kBlock)), dim3(kBlock), 0, st, c.idx, c.dig, c.n, cx.head.as<u64>(), parents, z, P, idx, dig);
        ++cx.launches;
        d.lv[l] = LevelView{idx, dig, parents};
        *permutations += parents;
    }
    const int levels = H - l + 1;  // >= 1: level H - 1 has at most two nodes
    d.bufs.emplace_back(new DeviceBuf);
    DeviceBuf& b = *d.bufs.back();
    PW_HIP_TRY((hipError_t)b.ensure((size_t)levels * kTail * 40));
    uint32_t* dig = b.as<uint32_t>();
    u64* idx = reinterpret_cast<u64*>(dig + (size_t)levels * kTail * 8);
    u64* d_counts = cx.small.as<u64>() + kTailCounts;
    const TailArgs a{d.lv[l - 1].idx, d.lv[l - 1].dig, d.lv[l - 1].n, l, H, idx, dig, d_counts, tree->zbuf.as<uint32_t>()};
    {
        ScopedKernelTimer t("memory_tree_tail_kernel");
        hipLaunchKernelGGL(tail_kernel<true>, dim3(1), dim3(kTail), 0, st, a, P);
    }
    ++cx.launches;
    u64 counts[kMaxHeight + 1];
    PW_HIP_TRY(hipMemcpyAsync(counts, d_counts, (size_t)levels * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipMemcpyAsync(d.root, dig + (size_t)(levels - 1) * kTail * 8, 32, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    for (int k = l; k <= H; ++k) {
        d.lv[k] = LevelView{idx + (size_t)(k - l) * kTail, dig + (size_t)(k - l) * kTail * 8, counts[k - l]};
        *permutations += counts[k - l];
    }
    return (int)hipGetLastError();
}

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" PwMemoryTree* pw_memory_tree_create(uint32_t height) {
    if (height < 1 || height > (uint32_t)kMaxHeight) return nullptr;
    PwMemoryTree* t = new PwMemoryTree;
    t->height = height;
    const p2::Params& p = poseidon2_params_host();
    memcpy(t->ext_rc, p.ext_rc, sizeof t->ext_rc);
    memcpy(t->int_rc, p.int_rc, sizeof t->int_rc);
    uint32_t st[16] = {0};
    pw_poseidon2_permute_host(st);  // canonical in and out: Z_0 = the digest of the zero payload
    for (int k = 0; k < 8; ++k) t->zero[0][k] = bb::to_monty(st[k]);
    for (uint32_t l = 1; l <= height; ++l) {
        for (int k = 0; k < 8; ++k) st[k] = st[8 + k] = bb::from_monty(t->zero[l - 1][k]);
        pw_poseidon2_permute_host(st);
        for (int k = 0; k < 8; ++k) t->zero[l][k] = bb::to_monty(st[k]);
    }
    t->data.lv.assign(height + 1, LevelView{nullptr, nullptr, 0});
    memcpy(t->data.root, t->zero[height], 32);
    return t;
}

extern "C" void pw_memory_tree_destroy(PwMemoryTree* tree) { delete tree; }

extern "C" int pw_memory_tree_root(const PwMemoryTree* tree, uint32_t* out) {
    if (!tree || !out || !same_table(tree)) return -1;
    for (int k = 0; k < 8; ++k) out[k] = bb::from_monty(tree->data.root[k]);
    return 0;
}

extern "C" int pw_memory_tree_stats(const PwMemoryTree* tree, PwMemoryTreeStats* out) {
    if (!tree || !out || !same_table(tree)) return -1;
    *out = PwMemoryTreeStats{tree->data.lv[0].n, tree->data.nodes, tree->data.bytes + tree->zbuf.bytes, tree->last_permutations, tree->last_launches,
                             tree->last_scratch};
    return 0;
}

extern "C" int pw_memory_tree_set_mode(PwMemoryTree* tree, uint32_t mode) {
    if (!tree || (mode != PW_MEMORY_TREE_REBUILD && mode != PW_MEMORY_TREE_INCREMENTAL) || !same_table(tree)) return -1;
    tree->mode = mode;
    return 0;
}

extern "C" int pw_memory_tree_get_mode(const PwMemoryTree* tree, uint32_t* mode) {
    if (!tree || !mode || !same_table(tree)) return -1;
    *mode = tree->mode;
    return 0;
}

extern "C" int pw_memory_tree_update(PwMemoryTree* tree, const uint64_t* d_keys_, const uint32_t* d_init, const uint32_t* d_fin, size_t n,
                                     uint32_t* d_records, uint64_t* d_node_ids_, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_rows,
                                     uint32_t* status, uint64_t* info) {
    if (!tree || !status || !info || (n && (!d_keys_ || !d_fin)) || !same_table(tree)) return -1;
    if (!d_init && (d_records || d_node_ids_)) return -1;       // load mode writes no records
    if (d_init && (!log_height || !n_rows)) return -1;
    if (d_node_ids_ && !d_records) return -1;
    if (d_records && (cap_log_height < 1 || cap_log_height > 40)) return -1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (tree->device >= 0 && tree->device != dev) return -1;
    (void)hipGetLastError();
    const u64* d_keys = reinterpret_cast<const u64*>(d_keys_);
    u64* d_node_ids = reinterpret_cast<u64*>(d_node_ids_);
    *status = 0;
    *info = 0;
    if (log_height) *log_height = 1;
    if (n_rows) *n_rows = 0;
    hipStream_t st = stream();
    if (!n) {  // nothing touched: no rows, the tree stays
        if (d_records) PW_HIP_TRY(hipMemsetAsync(d_records, 0, (size_t)25 * 2 * 4, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        tree->last_permutations = tree->last_launches = tree->last_scratch = 0;
        return 0;
    }
    TreeCtx& cx = g_tree;
    const ScratchCall call(cx);
    const int H = (int)tree->height;
    PW_HIP_TRY((hipError_t)cx.small.ensure(kSmallWords * 8));
    if (!tree->zbuf.p) {
        PW_HIP_TRY((hipError_t)tree->zbuf.ensure((size_t)(H + 1) * 32));
        PW_HIP_TRY(hipMemcpyAsync(tree->zbuf.p, tree->zero, (size_t)(H + 1) * 32, hipMemcpyHostToDevice, st));
        tree->device = dev;
    }
    const PwMemoryTree::Data& old = tree->data;
    const p2::Params& P = poseidon2_params_host();
    u64* d_err = cx.small.as<u64>() + kErr;
    u64 err[4] = {kNoIndex, kNoIndex, kNoIndex, kNoIndex};
    // 1. validate
    PW_HIP_TRY(hipMemcpyAsync(d_err, err, sizeof err, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(validate_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, st, d_keys, d_init, d_fin, (u64)n, (uint32_t)H, d_err);
    ++cx.launches;
    PW_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof err, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    if (err[0] != kNoIndex) { *status = 4; *info = err[0]; return 0; }
    if (err[1] != kNoIndex) { *status = 5; *info = err[1]; return 0; }
    // 2. continuity, and which keys are stored leaves already (before[j] = how many of the keys below j; before[n] = all of them)
    PW_HIP_TRY((hipError_t)cx.found.ensure((n + 1) * 8));
    PW_HIP_TRY((hipError_t)cx.before.ensure((n + 1) * 8));
    hipLaunchKernelGGL(lookup_kernel, dim3(div_up(n + 1, kBlock)), dim3(kBlock), 0, st, d_keys, d_init, (u64)n, old.lv[0], old.payload, cx.found.as<u64>(), d_err);
    ++cx.launches;
    PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
        return rocprim::exclusive_scan(t, b, cx.found.as<u64>(), cx.before.as<u64>(), 0ull, n + 1, rocprim::plus<u64>(), st);
    }));
    ++cx.launches;
    u64 n_found = 0;
    PW_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof err, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipMemcpyAsync(&n_found, cx.before.as<u64>() + n, 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    if (err[2] != kNoIndex) { *status = 3; *info = err[2]; return 0; }
    // 3. the records: index work only
    std::vector<u64> sizes;
    u64 phase_rows = 0;
    const bool incremental = d_init && tree->mode == PW_MEMORY_TREE_INCREMENTAL;  // load mode is the full rebuild in both modes
    if (d_init) {
        PW_TRY(touched_levels(cx, tree, d_keys, n, sizes, nullptr, incremental));
        for (u64 s : sizes) phase_rows += s;
        *n_rows = 2 * phase_rows;
        *log_height = ceil_log2_at_least_1(2 * phase_rows);
        if (d_records && cap_log_height < *log_height) { *status = 1; return 0; }
    }
    // 4. the new tree, next to the old one
    PwMemoryTree::Data fresh;
    fresh.lv.assign(H + 1, LevelView{nullptr, nullptr, 0});
    uint64_t permutations = n;
    {
        const u64 n0 = old.lv[0].n + n - n_found;
        fresh.bufs.emplace_back(new DeviceBuf);
        DeviceBuf& b = *fresh.bufs.back();
        PW_HIP_TRY((hipError_t)b.ensure((size_t)n0 * 72));
        uint32_t* dig = b.as<uint32_t>();
        uint32_t* payload = dig + (size_t)n0 * 8;
        u64* idx = reinterpret_cast<u64*>(payload + (size_t)n0 * 8);
        {
            ScopedKernelTimer t("memory_tree_leaf_kernel");
            hipLaunchKernelGGL(merge_new_kernel, dim3(div_up(n, kBlock)), dim3(kBlock), 0, st, d_keys, d_fin, (u64)n, old.lv[0], cx.before.as<u64>(), P, idx, payload, dig);
        }
        ++cx.launches;
        if (old.lv[0].n) {
            hipLaunchKernelGGL(merge_old_kernel, dim3(div_up(old.lv[0].n, kBlock)), dim3(kBlock), 0, st, d_keys, (u64)n, old.lv[0], old.payload, cx.before.as<u64>(), idx,
                               payload, dig);
            ++cx.launches;
        }
        fresh.lv[0] = LevelView{idx, dig, n0};
        fresh.payload = payload;
    }
    PW_TRY(build_levels(cx, tree, old, fresh, incremental ? &sizes : nullptr, &permutations));
    // phase-0 rows from the tree as it stands, phase-1 rows from the new one
    if (d_init && d_records) {
        const u64 pitch = (u64)1 << *log_height;
        PW_HIP_TRY(hipMemsetAsync(d_records, 0, (size_t)25 * pitch * 4, st));
        RecArgs rec{};
        for (int l = 0; l <= H; ++l) { rec.tree[0][l] = old.lv[l]; rec.tree[1][l] = fresh.lv[l]; }
        rec.payload[0] = old.payload; rec.payload[1] = fresh.payload;
        u64 row = 0;
        for (int l = 0; l <= H; ++l) { rec.lv[l].row = row; row += sizes[l]; }
        rec.phase_rows = phase_rows; rec.pitch = pitch; rec.rec = d_records; rec.ids = d_node_ids; rec.zero = tree->zbuf.as<uint32_t>();
        PW_TRY(touched_levels(cx, tree, d_keys, n, sizes, &rec));
    }
    PW_HIP_TRY(hipStreamSynchronize(st));
    PW_HIP_TRY(hipGetLastError());
    fresh.nodes = 0;
    fresh.bytes = 0;
    for (const LevelView& v : fresh.lv) fresh.nodes += v.n;
    for (const auto& b : fresh.bufs) fresh.bytes += b->bytes;
    std::swap(tree->data, fresh);
    tree->last_permutations = permutations;
    tree->last_launches = cx.launches;
    tree->last_scratch = cx.peak();
    return 0;
}

extern "C" int pw_memory_tree_open(const PwMemoryTree* tree_, const uint64_t* d_keys_, size_t n, uint32_t* d_payloads, uint32_t* d_siblings, uint64_t cap_siblings,
                                   uint64_t* n_siblings, uint32_t* status, uint64_t* info) {
    if (!tree_ || !d_keys_ || !n || !d_payloads || !d_siblings || !n_siblings || !status || !info || !same_table(tree_)) return -1;
    const int H = (int)tree_->height;
    const u64 lanes = (u64)n * (u64)H;
    if (n > ((u64)1 << 40) || div_up(n, kBlock) > 0x7fffffffu) return -1;  // more keys than leaves, or than one launch holds
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return -1; }
    if (tree_->device >= 0 && tree_->device != dev) return -1;
    (void)hipGetLastError();
    PwMemoryTree* tree = const_cast<PwMemoryTree*>(tree_);  // (Z_0 .. Z_H go to the device with the first call that needs them, as in the update)
    const u64* d_keys = reinterpret_cast<const u64*>(d_keys_);
    *status = 0;
    *info = 0;
    *n_siblings = 0;
    hipStream_t st = stream();
    TreeCtx& cx = g_tree;
    PW_HIP_TRY((hipError_t)cx.small.ensure(kSmallWords * 8));
    if (!tree->zbuf.p) {
        PW_HIP_TRY((hipError_t)tree->zbuf.ensure((size_t)(H + 1) * 32));
        PW_HIP_TRY(hipMemcpyAsync(tree->zbuf.p, tree->zero, (size_t)(H + 1) * 32, hipMemcpyHostToDevice, st));
        tree->device = dev;
    }
    // one scratch buffer, freed on every path: the scan's temporary storage | the ranks | the flags (the first two at 256-byte offsets,
    // the alignment of an allocation: rocPRIM lays its look-back state out from the start of what it is given)
    const FlagToCount to_u64{};
    DeviceBuf scratch;
    size_t temp_bytes = 0;
    const size_t rank_bytes = (size_t)(lanes + 1) * 8;
    {
        const auto none = rocprim::make_transform_iterator((const uint8_t*)nullptr, to_u64);
        PW_HIP_TRY(rocprim::exclusive_scan(nullptr, temp_bytes, none, (u64*)nullptr, 0ull, (size_t)(lanes + 1), rocprim::plus<u64>(), st));
    }
    const size_t temp_room = (std::max<size_t>(temp_bytes, 16) + 255) & ~(size_t)255;
    PW_HIP_TRY((hipError_t)scratch.ensure(temp_room + rank_bytes + (size_t)(lanes + 1)));
    void* d_temp = scratch.p;
    u64* d_rank = reinterpret_cast<u64*>(scratch.as<uint8_t>() + temp_room);
    uint8_t* d_flags = scratch.as<uint8_t>() + temp_room + rank_bytes;
    u64* d_err = cx.small.as<u64>() + kErr;
    u64 err = kNoIndex, total = 0;
    const dim3 grid(div_up(n, kBlock), H);
    PW_HIP_TRY(hipMemcpyAsync(d_err, &err, 8, hipMemcpyHostToDevice, st));
    {
        ScopedKernelTimer t("memory_tree_open_flag_kernel");
        hipLaunchKernelGGL(open_flag_kernel, grid, dim3(kBlock), 0, st, d_keys, (u64)n, (uint32_t)H, d_flags, d_err);
    }
    {
        ScopedKernelTimer t("memory_tree_open_scan");
        PW_HIP_TRY(rocprim::exclusive_scan(d_temp, temp_bytes, rocprim::make_transform_iterator((const uint8_t*)d_flags, to_u64), d_rank, 0ull, (size_t)(lanes + 1),
                                           rocprim::plus<u64>(), st));
    }
    PW_HIP_TRY(hipMemcpyAsync(&err, d_err, 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipMemcpyAsync(&total, d_rank + lanes, 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    if (err != kNoIndex) { *status = 4; *info = err; return 0; }
    if (total > lanes) return -1;
    *n_siblings = total;
    if (total > cap_siblings) { *status = 1; return 0; }
    OpenArgs a{};
    for (int l = 0; l < H; ++l) a.lv[l] = tree->data.lv[l];
    a.payload = tree->data.payload;
    a.zero = tree->zbuf.as<uint32_t>();
    {
        ScopedKernelTimer t("memory_tree_open_gather_kernel");
        hipLaunchKernelGGL(open_gather_kernel, grid, dim3(kBlock), 0, st, a, d_keys, (u64)n, (const uint8_t*)d_flags, (const u64*)d_rank, d_payloads, d_siblings);
    }
    PW_HIP_TRY(hipStreamSynchronize(st));
    return (int)hipGetLastError();
}

extern "C" int pw_memory_tree_boundary_leaves(const uint32_t* d_boundary_trace, uint32_t log_height, uint64_t n_locations, uint64_t* d_keys, uint32_t* d_init,
                                              uint32_t* d_fin) {
    if (!d_boundary_trace || log_height < 1 || log_height > 40 || n_locations > ((uint64_t)1 << log_height) || (n_locations && (!d_keys || !d_init || !d_fin))) return -1;
    (void)hipGetLastError();
    hipStream_t st = stream();
    if (n_locations)
        hipLaunchKernelGGL(boundary_leaves_kernel, dim3(div_up(n_locations, kBlock)), dim3(kBlock), 0, st, d_boundary_trace, (u64)1 << log_height, (u64)n_locations,
                           reinterpret_cast<u64*>(d_keys), d_init, d_fin);
    PW_HIP_TRY(hipStreamSynchronize(st));
    return (int)hipGetLastError();
}
