// What the routines that walk a segment's bus interactions on raw traces share — the bus mock prover (bus_check.hip),
// the generators of the system AIRs' traces (system_traces.hip, §5j, §5l) and the empirical-constraint detector (empirical.hip, §5p):
// the packed witness and its codec, the open-addressing table (the claim loop on the device; the sizing rule and the
// grow-until-it-holds loop on the host: the ONE place either is written), the head of a walker's `small` buffer, the AIRs on a bus
// with their interactions ordered by bus, the staging of preprocessed provers. (The kernel that re-evaluates the tuples witnesses
// name: bus_witness_args.hpp.) Not part of the C ABI.
#pragma once
#include "prover_state.hpp"
#include "logup_eval.hpp"

#include <algorithm>
#include <type_traits>
#include <vector>

namespace pw {
namespace bus {

constexpr int kBlock = kLogupBlock;
constexpr int kWaves = kBlock / 64;
typedef unsigned long long u64;

constexpr u64 kEmpty = ~0ull;          // a key half no fingerprint can be (its words are below 2^31)
constexpr uint32_t kRowBits = 26, kInterBits = 20, kAirBits = 18;  // the packed witness (air | interaction | row)
constexpr size_t kSlotBytes = 40;      // key 2 x 8, sum 8, witness 8, count 8
constexpr u64 kStartSlots = 1ull << 16;  // the first table of a bus (2.6 MB); quadrupled on overflow up to the bound
// A table counts as full at 7/8 of its slots, so that linear probing stays short however the bound was chosen: the slots fall into
// up to 64 classes (slot index mod the class count, at least 4096 slots each), every class counts the slots claimed in it (counters
// 256 bytes apart: one atomic per DISTINCT tuple, spread over the memory channels) and the bus overflows when a class passes 7/8.
constexpr u64 kMaxClasses = 64, kMinClassSlots = 4096, kLoadStride = 32;

// the interactions order[begin .. end) of an AIR are those on selected bus number `slot`
struct BusSeg { uint32_t begin, end, slot, pad; };
// what a kernel that re-evaluates a witness's tuple needs of an AIR
struct AirDev { const uint32_t* m; u64 H; LogupProgram lp; };

struct Witness { uint32_t air, inter; size_t row; };
__host__ __device__ __forceinline__ u64 pack_witness(uint32_t air, uint32_t inter, size_t row) {
    return ((u64)air << (kRowBits + kInterBits)) | ((u64)inter << kRowBits) | (u64)row;
}
__host__ __device__ __forceinline__ Witness unpack_witness(u64 w) {
    return Witness{(uint32_t)(w >> (kRowBits + kInterBits)), (uint32_t)(w >> kRowBits) & ((1u << kInterBits) - 1u), (size_t)(w & ((1ull << kRowBits) - 1ull))};
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ u64 wave_min(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

// a 64-bit sum of centred multiplicities (two's complement) as its canonical residue mod p
__device__ __forceinline__ uint32_t sum_residue(u64 sum) {
    long long v = (long long)sum % (long long)bb::P;
    if (v < 0) v += (long long)bb::P;
    return (uint32_t)v;
}

// the span on row r, by the program's small forms where it has them (the choice a host launch makes with with_fast)
__device__ __forceinline__ uint32_t eval_span_of(const AirDev& a, uint32_t span, size_t r, uint32_t* stk) {
    return a.lp.d_forms ? eval_span<true>(a.lp, span, a.m, (size_t)a.H, r, stk) : eval_span<false>(a.lp, span, a.m, (size_t)a.H, r, stk);
}

__device__ __forceinline__ u64 slot_hash(u64 a, u64 b) {
    u64 h = a * 0x9E3779B97F4A7C15ull ^ (b + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

// ---- the open-addressing table: device side --------------------------------------------------------------------------------------
// What every table here has, whatever its payload columns: the slot mask and the class accounting of the load rule above
// (table_rule below derives them from the slots), and one or two 64-bit key columns (k1 unused by a one-word key).
struct TableRule { u64 mask; u64* load; u64 class_mask, class_cap; };
struct TableView : TableRule { u64 *k0, *k1; };

// where a key's probe starts: a two-word key hashes as its words, a one-word key (as << 32 | ptr) as (as, ptr)
template <int WORDS>
__device__ __forceinline__ u64 key_hash(u64 a, u64 b) { return WORDS == 2 ? slot_hash(a, b) : slot_hash(a >> 32, a & 0xffffffffull); }

// The slot that holds key (a, b) (WORDS = 1: a alone), claimed if no slot held it yet; kEmpty, with *overflow set, when there is
// none. Linear probing from the key's hash; each key word is claimed by a compare-and-swap (after a plain load: most probes meet a
// word that is set); a slot whose first word matches and whose second does not belongs to another key: keep probing. Keys never
// change once set, so every contribution of a key ends in the same slot whatever the order of arrival. The lane that claims a fresh
// slot counts it in the slot's class; a class past its cap sets *overflow, and so does a lane that has seen every slot taken by
// other keys (only tables of fewer than 8 slots get that far). With linear probing the SET of taken slots does not depend on the
// order of arrival and only grows with the keys inserted, so whether a class passes its cap — *overflow — is a function of the
// traces and the table size alone. A lane gives up every 64 probes once it is set: the host throws the table away.
template <int WORDS>
__device__ __forceinline__ u64 claim_slot(const TableView& t, u64 a, u64 b, uint32_t* __restrict__ overflow) {
    const u64 h = key_hash<WORDS>(a, b);
    for (u64 n = 0; n <= t.mask; ++n) {
        const u64 s = (h + n) & t.mask;
        u64 ka = __atomic_load_n(t.k0 + s, __ATOMIC_RELAXED);
        if (ka == kEmpty) {
            ka = atomicCAS(t.k0 + s, kEmpty, a);
            if (ka == kEmpty) {
                ka = a;
                if (atomicAdd(t.load + (s & t.class_mask) * kLoadStride, 1ull) >= t.class_cap) atomicOr(overflow, 1u);
            }
        }
        if (ka == a) {
            if (WORDS == 1) return s;
            u64 kb = __atomic_load_n(t.k1 + s, __ATOMIC_RELAXED);
            if (kb == kEmpty) {
                kb = atomicCAS(t.k1 + s, kEmpty, b);
                if (kb == kEmpty) kb = b;
            }
            if (kb == b) return s;
        }
        if ((n & 63) == 63 && __atomic_load_n(overflow, __ATOMIC_RELAXED)) break;
    }
    atomicOr(overflow, 1u);
    return kEmpty;
}

// the slot that holds the one-word key, or kEmpty: read-only, after the walk that claimed
__device__ __forceinline__ u64 find_slot(const TableView& t, u64 key) {
    const u64 h = key_hash<1>(key, 0);
    for (u64 n = 0; n <= t.mask; ++n) {
        const u64 s = (h + n) & t.mask;
        const u64 k = __atomic_load_n(t.k0 + s, __ATOMIC_RELAXED);
        if (k == key) return s;
        if (k == kEmpty) break;
    }
    return kEmpty;
}

// ---- host --------------------------------------------------------------------------------------------------------------------------

#define PW_TRY(x) do { const int _rc = (x); if (_rc) return _rc; } while (0)

// the list of AIRs every entry point here takes: false = malformed (refused before any GPU call)
inline bool airs_well_formed(const PwSegmentAir* airs, size_t n_airs) {
    if ((!airs && n_airs) || n_airs >= ((size_t)1 << kAirBits)) return false;
    std::vector<const PwProver*> pre;
    for (size_t a = 0; a < n_airs; ++a) {
        const PwProver* p = airs[a].prover;
        if (!p || !airs[a].d_trace || airs[a].log_height > kRowBits) return false;
        if (p->pre_width && airs[a].log_height != p->pre_log_h) return false;
        if (p->logup && p->n_inter >= (1u << kInterBits)) return false;
        if (p->pre_width) pre.push_back(p);
    }
    std::sort(pre.begin(), pre.end());
    return std::adjacent_find(pre.begin(), pre.end()) == pre.end();  // one staging matrix cannot hold two traces
}

// the prover's interactions ordered by (bus id, index), once per prover
inline int ensure_bus_order(PwProver* p) {
    if (!p->h_bus_starts.empty() || !p->n_inter) return 0;
    std::vector<uint32_t> order(p->n_inter);
    for (uint32_t i = 0; i < p->n_inter; ++i) order[i] = i;
    auto bus_of = [&](uint32_t i) { return bb::from_monty(p->h_inter[i].bus_monty); };
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return bus_of(x) < bus_of(y); });
    std::vector<uint32_t> ids, starts;
    for (uint32_t k = 0; k < p->n_inter; ++k)
        if (!k || bus_of(order[k]) != bus_of(order[k - 1])) { ids.push_back(bus_of(order[k])); starts.push_back(k); }
    starts.push_back(p->n_inter);
    PW_TRY(p->bus_order.ensure(order.size() * 4));
    PW_HIP_TRY(hipMemcpy(p->bus_order.p, order.data(), order.size() * 4, hipMemcpyHostToDevice));
    p->h_bus_order = std::move(order);
    p->h_bus_ids = std::move(ids);
    p->h_bus_starts = std::move(starts);
    return 0;
}

inline LogupProgram program_of(const PwProver* p) {
    return LogupProgram{p->d_inter, p->n_inter, p->d_ixspans, p->d_icode, p->d_gstarts, p->n_groups, p->d_iforms};
}

// what the interaction programs of AIR a read: the trace, or with preprocessed columns the prover's (trace | fixed) staging matrix
// (one copy per call: the argument check refuses a preprocessed prover that occurs twice, whose two traces would share the matrix)
inline int stage_values(const PwSegmentAir& a, const uint32_t** out) {
    PwProver* p = a.prover;
    *out = a.d_trace;
    if (!p->pre_width) return 0;
    const size_t H = (size_t)1 << a.log_height;
    PW_HIP_TRY(hipMemcpyAsync(p->pre_vals.as<uint32_t>(), a.d_trace, (size_t)p->width * H * 4, hipMemcpyDeviceToDevice, stream()));
    *out = p->pre_vals.as<uint32_t>();
    return 0;
}

// an AIR that has interactions on a bus: their run in the prover's bus order and the values its programs read
struct Part { size_t air; uint32_t begin, end; const uint32_t* vals; };

// THE rule for "this AIR is on `bus`": how many interactions its prover has there (0 = it takes no part). Whatever lists, counts or
// numbers the AIRs of a bus asks here. *same_arity, where given, is cleared by an interaction on the bus that has not n_args arguments.
inline uint32_t interactions_on(const PwProver* p, uint32_t bus, uint32_t n_args = 0, bool* same_arity = nullptr) {
    uint32_t n = 0;
    if (!p->logup) return 0;
    for (const LogupInteraction& it : p->h_inter)
        if (bb::from_monty(it.bus_monty) == bus) {
            if (same_arity && it.n_args != n_args) *same_arity = false;
            ++n;
        }
    return n;
}

// the parts of `bus` in AIR order, their values staged, and with `air_tab` the table a kernel that re-evaluates witnesses reads
inline int collect_parts(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, std::vector<Part>& parts, std::vector<AirDev>* air_tab) {
    if (air_tab) air_tab->assign(n_airs, AirDev{nullptr, 0, LogupProgram{}});
    for (size_t a = 0; a < n_airs; ++a) {
        PwProver* p = airs[a].prover;
        if (!interactions_on(p, bus)) continue;
        PW_TRY(ensure_bus_order(p));
        const size_t k = std::lower_bound(p->h_bus_ids.begin(), p->h_bus_ids.end(), bus) - p->h_bus_ids.begin();  // (there: the order lists every bus)
        Part part{a, p->h_bus_starts[k], p->h_bus_starts[k + 1], nullptr};
        PW_TRY(stage_values(airs[a], &part.vals));
        if (air_tab) (*air_tab)[a] = AirDev{part.vals, (u64)1 << airs[a].log_height, program_of(p)};
        parts.push_back(part);
    }
    return 0;
}

// what a walk over the rows of an AIR is launched with
struct Walked { size_t H; LogupProgram lp; const uint32_t* order; };
inline Walked walked(const PwSegmentAir& a) { return Walked{(size_t)1 << a.log_height, program_of(a.prover), (const uint32_t*)a.prover->bus_order.p}; }

// f(std::true_type) where the program has small forms (the kernel's FAST = true), f(std::false_type) where not: a launch written
// once as hipLaunchKernelGGL(kernel<decltype(fast)::value>, ...) covers both
template <class F>
inline void with_fast(const LogupProgram& lp, F&& f) {
    if (lp.d_forms) f(std::true_type{});
    else f(std::false_type{});
}

// a fixed stream of challenges: splitmix64, four words below p
inline uint64_t splitmix(uint64_t& s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline bb::Ext challenge(uint64_t& s) {
    bb::Ext e;
    for (int k = 0; k < 4; ++k) e.c[k] = bb::to_monty((uint32_t)(splitmix(s) % bb::P));
    return e;
}

// ---- the open-addressing table: host side ----------------------------------------------------------------------------------------
// the bound of a table or a scratch area whose caller gave none: half of what the device has room for
inline size_t default_bound(size_t held) {
    size_t avail = 0;
    return device_room(held, &avail) ? avail / 2 : (size_t)1 << 30;
}

// The head of a walker's `small` buffer, as it lies on the device: what the counting compact leaves (four counters, each walker's
// own), the overflow word and the walker's flags — read back together after every table — and the class loads.
struct WalkCounts { u64 counts[4] = {0, 0, 0, 0}; uint32_t overflow = 1, flags = 0, pad[2] = {0, 0}; };
struct WalkHead { WalkCounts c; u64 load[kMaxClasses * kLoadStride]; };
static_assert(sizeof(WalkCounts) == 48 && sizeof(WalkHead) == 48 + kMaxClasses * kLoadStride * 8, "no padding: the head is cleared and read back as bytes");

inline TableRule table_rule(u64 slots, WalkHead* d_head) {
    const u64 classes = std::min<u64>(kMaxClasses, std::max<u64>(1, slots / kMinClassSlots)), per_class = slots / classes;
    return TableRule{slots - 1, d_head->load, classes - 1, per_class - per_class / 8};
}

struct Grown {
    u64 slots = 0;         // of the last table walked
    WalkCounts c;          // read back after it (overflow = 1 while there is none)
    uint64_t tables = 0;   // tables walked, those that overflowed included
    bool no_table = true;  // the bound holds not one slot, or the device gave none
    bool overflowed() const { return c.overflow != 0; }  // at the bound: not localised
};

// The sizing rule and the growth of every table here. The largest table is a power of two of slots, at most twice the triples walked
// (no walk needs more) and within `bound` bytes. The first has `first_slots`; while a walk overflows its table the next is four
// times as large, up to the largest: lookup buses repeat a few hundred thousand tuples thousands of times, so the triples say little
// about the table a walk needs, and an overflowing walk stops early (every lane leaves once the overflow word is set). What comes
// out depends on the LAST table alone. A table the device cannot give is a table too large: try half, never an error.
//   table            the walker's buffer, a Scratch::Buf (scratch.hpp): every table it becomes is noted in the context's peak
//   clear(tb, rule)  the table at tb, of rule.mask + 1 slots, is the caller's from here on: bind its columns and issue their
//                    0xFF / 0 patterns (timed as `clear_timer` together with the clearing of the head)
//   walk()           the claiming kernels
//   count()          the counting launch of the caller's compact kernel, into d_head->c.counts
template <class Table, class Clear, class Walk, class Count>
inline int grow_table(Table& table, WalkHead* d_head, u64 triples, size_t slot_bytes, size_t bound, u64 first_slots, const char* clear_timer, Clear clear,
                      Walk walk, Count count, Grown* g) {
    *g = Grown{};
    u64 max_slots = 1024;
    while (max_slots < 2 * triples) max_slots <<= 1;
    while (max_slots && max_slots * slot_bytes > bound) max_slots >>= 1;
    if (!max_slots) return 0;
    hipStream_t st = stream();
    u64 slots = std::min(max_slots, first_slots);
    for (;;) {
        int erc;
        while ((erc = table.ensure(slots * slot_bytes)) != 0) {
            (void)hipGetLastError();
            if (erc != (int)hipErrorOutOfMemory) return erc;
            if (slots <= 1) break;
            max_slots = slots >>= 1;
        }
        if (!table.p) break;
        {
            ScopedKernelTimer timer(clear_timer);
            PW_TRY(clear(table.template as<u64>(), table_rule(slots, d_head)));
            PW_HIP_TRY(hipMemsetAsync(d_head, 0, sizeof(WalkHead), st));
        }
        walk();
        count();
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipMemcpyAsync(&g->c, d_head, sizeof(WalkCounts), hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        ++g->tables;
        if (!g->c.overflow || slots >= max_slots) break;
        slots = std::min(max_slots, slots * 4);
    }
    g->slots = slots;
    g->no_table = !table.p;
    return 0;
}


}  // namespace bus
}  // namespace pw
