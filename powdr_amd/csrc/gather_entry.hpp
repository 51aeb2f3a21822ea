// What the gather entries (_apc_tracegen, powdr_apc_tracegen_host_tables, _callmajor, _records) share besides the plan cache.
// Not part of the C ABI.
#pragma once
#include "common.hpp"

#include <unordered_map>
#include <vector>

namespace pw {

// How every gather entry opens: the sticky error of an unrelated earlier call is dropped, H must be a power of two (reference:
// assert, apc_tracegen.cu:134), empty input is finished at once, and the call count is clamped to [0, H] (rows r >= H do not
// exist; nullptr: the entry has a rule of its own). Returns kGatherProceeds or the code the entry returns at once.
constexpr int kGatherProceeds = -1;
inline int gather_opening(size_t H, size_t n_subs, int* num_apc_calls) {
    (void)hipGetLastError();
    if ((H & (H - 1)) != 0) return (int)hipErrorInvalidValue;
    if (H == 0 || n_subs == 0) return (int)hipGetLastError();
    if (num_apc_calls) {
        if (*num_apc_calls < 0) *num_apc_calls = 0;
        if ((size_t)*num_apc_calls > H) *num_apc_calls = (int)H;
    }
    return kGatherProceeds;
}

// Duplicate destinations resolve like the reference's sequential loop: the last substitution for an APC column wins.
// apc_col(i) = the destination of entry i; keep[i] = 1 for the entries that survive.
template <class ApcCol>
std::vector<char> last_wins(size_t n, ApcCol apc_col) {
    std::vector<char> keep(n, 1);
    std::unordered_map<int32_t, size_t> last;
    last.reserve(n * 2);
    for (size_t i = 0; i < n; ++i) {
        auto ins = last.emplace(apc_col(i), i);
        if (!ins.second) { keep[ins.first->second] = 0; ins.first->second = i; }
    }
    return keep;
}

}  // namespace pw
