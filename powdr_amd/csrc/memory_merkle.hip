// The memory Merkle AIR's trace (include/powdr_prover.h pw_memory_merkle_trace; the AIR: powdr_amd/memory_tree.py
// merkle_air): the record rows of one pw_memory_tree_update — every touched node twice, before the segment (phase 0) and after it
// (phase 1), in the same node order — folded into ONE row per node, the root first.
//   merkle_rows_kernel  one lane per output row. Row r is node j = n_nodes - 1 - r of the records order. Its two record rows are read
//                       column by column and the 55 columns written the same way: consecutive lanes touch consecutive words of one
//                       column (in descending order on the read side), so every load and store of a wave is one contiguous run.
//                       level and index come from the node id; the touched flags from ONE lower_bound for the left child's id
//                       (level - 1, 2 index) in the phase-0 half of the ids and a look at the entry after it: the ids are strictly
//                       increasing as 64-bit words, so the sibling is adjacent. Every output place is a function of the row number:
//                       no byte depends on an order of arrival. Rows past n_nodes are zero.
// THE COLUMN POSITIONS ARE THOSE OF MERKLE_COLUMNS (powdr_amd/memory_tree.py) and of the records (memory_tree.hip records_kernel:
// [valid, left[8], right[8], out[8]]) — they move together.
#include "prover_state.hpp"

namespace pw {

namespace {

typedef unsigned long long u64;
constexpr int kBlock = 256;
constexpr uint32_t kMaxMerkleHeight = 30;  // an index below 2^30 is a field element
constexpr uint32_t kMaxLogHeight = 38;     // of the records and of the trace: one lane per row, and 2^38 / kBlock workgroups fit a grid
constexpr uint32_t kRecordColumns = 25, kMerkleColumns = 55;
constexpr uint32_t kColValid = 0, kColIsRoot = 1, kColIsLeaf = 2, kColLeftTouched = 3, kColRightTouched = 4, kColLevel = 5, kColIndex = 6, kColWords = 7;
constexpr u64 kPhaseBit = 1ull << 63, kIndexMask = (1ull << 56) - 1ull;

__device__ __forceinline__ u64 lower_bound(const u64* __restrict__ a, u64 n, u64 key) {
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (a[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// bad[0] != 0 afterwards: the ids are not a records set (the phase-1 id of a node is not its phase-0 id with the phase bit set, a
// level above H or an index that does not fit its level, or the last node is not the root (H, 0)). Every access stays inside the
// buffers whatever the ids hold: the rows read are j and n_nodes + j, the search runs over ids[0 .. n_nodes).
__global__ __launch_bounds__(kBlock) void merkle_rows_kernel(const uint32_t* __restrict__ rec, u64 rec_pitch, const u64* __restrict__ ids, u64 n_nodes,
                                                              uint32_t H, u64 pitch, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
    const u64 r = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (r >= pitch) return;
    uint32_t* o = out + r;
    if (r >= n_nodes) {
#pragma unroll
        for (uint32_t c = 0; c < kMerkleColumns; ++c) o[(size_t)c * pitch] = 0u;
        return;
    }
    const u64 j = n_nodes - 1 - r;
    const u64 id = ids[j];
    const uint32_t level = (uint32_t)((id & ~kPhaseBit) >> 56);
    const u64 index = id & kIndexMask;
    const bool root = id == ((u64)H << 56);
    bool wrong = ids[n_nodes + j] != (id | kPhaseBit) || (id & kPhaseBit) != 0 || level > H || (index >> (H - (level > H ? H : level))) != 0;
    if (r == 0) wrong |= !root;
    if (wrong) bad[0] = 1u;  // (every lane that writes writes the same word)
    bool left = false, right = false;
    if (level > 0) {
        const u64 child = ((u64)(level - 1) << 56) | ((2 * index) & kIndexMask);
        u64 c = lower_bound(ids, n_nodes, child);
        if (c < n_nodes && ids[c] == child) { left = true; ++c; }
        right = c < n_nodes && ids[c] == child + 1;
    }
    const uint32_t one = bb::R_MOD_P;
    o[(size_t)kColValid * pitch] = one;
    o[(size_t)kColIsRoot * pitch] = root ? one : 0u;
    o[(size_t)kColIsLeaf * pitch] = level == 0 ? one : 0u;
    o[(size_t)kColLeftTouched * pitch] = left ? one : 0u;
    o[(size_t)kColRightTouched * pitch] = right ? one : 0u;
    o[(size_t)kColLevel * pitch] = bb::to_monty(level & 0x3Fu);
    o[(size_t)kColIndex * pitch] = bb::to_monty((uint32_t)(index & 0x3FFFFFFFull));
    const uint32_t* before = rec + j;
    const uint32_t* after = rec + n_nodes + j;
#pragma unroll
    for (uint32_t k = 0; k < kRecordColumns - 1; ++k) {  // left, right, out: the record without its valid column
        o[(size_t)(kColWords + k) * pitch] = before[(size_t)(1 + k) * rec_pitch];
        o[(size_t)(kColWords + kRecordColumns - 1 + k) * pitch] = after[(size_t)(1 + k) * rec_pitch];
    }
}

}  // namespace

}  // namespace pw

using namespace pw;

extern "C" int pw_memory_merkle_trace(const uint32_t* d_records, uint32_t records_log_height, const uint64_t* d_node_ids, uint64_t n_rows, uint32_t height,
                                      uint32_t* d_trace_out, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_nodes, uint32_t* status) {
    if (!d_records || !d_node_ids || !d_trace_out || !log_height || !n_nodes || !status) return -1;
    if ((n_rows & 1) || height < 1 || height > kMaxMerkleHeight) return -1;
    if (records_log_height < 1 || records_log_height > kMaxLogHeight || n_rows > ((uint64_t)1 << records_log_height)) return -1;
    if (cap_log_height < 1 || cap_log_height > kMaxLogHeight) return -1;
    const u64 n = n_rows / 2;
    *n_nodes = n;
    *status = 0;
    uint32_t lh = 1;
    while (((u64)1 << lh) < n) ++lh;
    *log_height = lh;
    if (!n) { *status = 2; return 0; }  // a segment that touches no memory has no root row
    if (lh > cap_log_height) { *status = 1; return 0; }
    (void)hipGetLastError();
    hipStream_t st = stream();
    DeviceBuf flag;  // released on every path
    PW_HIP_TRY((hipError_t)flag.ensure(16));
    PW_HIP_TRY(hipMemsetAsync(flag.p, 0, 16, st));
    const u64 pitch = (u64)1 << lh;
    {
        ScopedKernelTimer timer("memory_merkle_rows_kernel");
        hipLaunchKernelGGL(merkle_rows_kernel, dim3(div_up(pitch, kBlock)), dim3(kBlock), 0, st, d_records, (u64)1 << records_log_height,
                           reinterpret_cast<const u64*>(d_node_ids), n, height, pitch, d_trace_out, flag.as<uint32_t>());
    }
    PW_HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    PW_HIP_TRY(hipMemcpyAsync(&bad, flag.p, 4, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    if (bad) *status = 3;
    return (int)hipGetLastError();
}
