// What the routines that walk a segment's bus interactions on raw traces share — the bus mock prover (bus_check.hip)
// and the generators of the system AIRs' traces (system_traces.hip, §5j): the packed witness, the open-addressing table's hashing and
// load rule, the provers' interactions ordered by bus, the staging of preprocessed provers. Not part of the C ABI.
#pragma once
#include "prover_state.hpp"
#include "logup_eval.hpp"

#include <algorithm>
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

__device__ __forceinline__ u64 pack_witness(uint32_t air, uint32_t inter, size_t row) {
    return ((u64)air << (kRowBits + kInterBits)) | ((u64)inter << kRowBits) | (u64)row;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ u64 slot_hash(u64 a, u64 b) {
    u64 h = a * 0x9E3779B97F4A7C15ull ^ (b + 0x632BE59BD9B4E019ull) * 0xC2B2AE3D27D4EB4Full;
    h ^= h >> 29;
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 32);
}

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


}  // namespace bus
}  // namespace pw
