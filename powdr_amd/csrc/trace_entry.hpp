// The entry contract of a pipeline that takes "the instruction-AIR traces of one execution" (DESIGN.md §5p), written once: what is
// refused with -1, which AIRs are on the bridge, what the time index needs and how it is opened. An entry point reads as
//   its own argument checks -> one_segment / calls_well_formed / airs_well_formed / bridge_of -> ScratchCall -> its status-2 bound ->
//   open -> its own stages (calls_within where it takes a call list).
// Not part of the C ABI.
#pragma once
#include "time_index.hpp"

namespace pw {
namespace time_index {

// the AIRs name one segment (candidates, calls and cuts end with their segment); NULL = segment 0 for all
inline bool one_segment(const uint32_t* segment_of_air, size_t n_airs) {
    if (segment_of_air)
        for (size_t a = 1; a < n_airs; ++a)
            if (segment_of_air[a] != segment_of_air[0]) return false;
    return true;
}

// false = -1: a NULL list, 2^31 or more APCs or calls, an APC of no cycles, a call of an APC there is not or of another length than
// its APC's cycle count, calls that are not ascending or overlap
inline bool calls_well_formed(const uint32_t* cycle_counts, size_t n_apcs, const uint32_t* ids, const uint64_t* from, const uint64_t* to, size_t n_calls) {
    if ((!cycle_counts && n_apcs) || ((!ids || !from || !to) && n_calls) || n_apcs >= ((size_t)1 << 31) || n_calls >= ((size_t)1 << 31)) return false;
    for (size_t a = 0; a < n_apcs; ++a)
        if (!cycle_counts[a]) return false;
    for (size_t j = 0; j < n_calls; ++j)
        if (ids[j] >= n_apcs || to[j] < from[j] || to[j] - from[j] != cycle_counts[ids[j]] || (j && from[j] < to[j - 1])) return false;
    return true;
}

// false with *status = 11 and *info = the first call that ends after the execution's N positions
inline bool calls_within(const uint64_t* to, size_t n_calls, u64 N, uint32_t* status, uint64_t* info) {
    for (size_t j = 0; j < n_calls; ++j)
        if (to[j] > N) {
            *status = 11;
            *info = j;
            return false;
        }
    return true;
}

// The AIRs on the bridge, by bus_shared.hpp's interactions_on — the rule collect_parts lists its parts by, so part k there is
// part_air[k] here: g0[k] = the global number of its first row (the parts' rows numbered through), M = g0[n_parts] = all their rows.
struct Bridge {
    std::vector<size_t> part_air;
    std::vector<int64_t> part_of_air;  // [n_airs], -1 = takes no part
    std::vector<u64> g0;               // [n_parts + 1]
    u64 M = 0;
    size_t n_parts() const { return part_air.size(); }
};
// false = -1: an interaction on the bridge with another arity than (pc, timestamp). The AIR list is well formed.
inline bool bridge_of(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, Bridge* b) {
    bool two_args = true;
    b->part_of_air.assign(n_airs, -1);
    b->g0.assign(1, 0);
    for (size_t a = 0; a < n_airs; ++a) {
        if (!interactions_on(airs[a].prover, bus, 2, &two_args)) continue;
        b->part_of_air[a] = (int64_t)b->part_air.size();
        b->part_air.push_back(a);
        b->g0.push_back(b->g0.back() + ((u64)1 << airs[a].log_height));
    }
    b->M = b->g0.back();
    return two_args;
}

// the bytes the index of M rows needs: the counters, 32 per row, the sort's temporary storage
inline size_t bytes_needed(u64 M) { return 64 + (size_t)M * 32 + (M ? sort_pairs_temp(M) : 0); }

// Opens the index of the bridge's rows: stages the parts' values (collect_parts: the first touch of the device, so after the status-2
// decision) and runs rows_in_time_order. *N = the active rows; *status = 7 or 4 with *info where the rows are no execution, then
// nothing else is valid. No row, nothing done. d_counters, counters: of a caller that counts on in them (rows_in_time_order).
inline int open(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, const Bridge& b, Stage& s, Scratch::Buf& temp, Names names, u64* N,
                uint32_t* status, uint64_t* info, u64* d_counters = nullptr, u64* counters = nullptr) {
    u64 own[8];
    if (!counters) counters = own;
    *N = 0;
    if (!b.M) return 0;
    std::vector<Part> parts;
    PW_TRY(collect_parts(airs, n_airs, bus, parts, nullptr));
    PW_TRY(rows_in_time_order(airs, segment_of_air, parts, b.g0, b.M, s, d_counters, temp, names, counters, status, info));
    if (!*status) *N = counters[0];
    return 0;
}

}  // namespace time_index
}  // namespace pw
