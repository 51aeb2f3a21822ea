// Applying APC calls on the device (include/powdr_prover.h pw_apc_sources_from_traces / pw_trace_gather_rows): from a
// segment's instruction-AIR traces and a list of non-overlapping calls (apc_id, from, to), per APC and original AIR the call-major
// source matrix _apc_tracegen reads (call r owns the rows row + r * row_block_size), and per AIR the residual trace: the active rows no
// call covers, compacted in row order.
//   index      time_index.hpp, unchanged: position i < N is the active row with the i-th smallest time key, idx_s[i] its global row
//   place      apc_sources_layout_kernel    one lane per covered position finds its call (binary search over the calls' covered
//                                           prefix): the first call of an APC writes the AIR of instruction k, every other call
//                                           compares its own with the first call's (status 12: atomicMin of the position)
//              (host)                       occ and rbs from the AIRs of the instructions: at most the sum of the cycle counts
//              apc_sources_place_kernel     the lane writes its local row into the index list of (apc, AIR) at call * rbs + occ and
//                                           a covered flag at its global row
//              apc_sources_keep_kernel      active && !covered per global row; an exclusive scan, cut at each AIR's first row
//              apc_sources_residual_kernel  gives the residual index lists
//              Index lists are cleared to 0xFFFFFFFF = "zero row" up to the output height: tails and gaps need no special case.
//   gather     apc_sources_gather_kernel    out[c * H_out + i] = idx[i] == ~0 ? 0 : in[c * H_in + idx[i]], ONE launch for all jobs:
//                                           a workgroup is (job, tile of kTileRows rows, group of kColGroup columns) and finds its
//                                           job by binary search over the jobs' first tiles. A lane owns 4 consecutive output rows:
//                                           one 16-byte load of its indices, reused over the columns of the group; every store is one
//                                           aligned 16-byte store; four consecutive source rows at a 16-byte aligned address are one
//                                           16-byte load (a chip fills its trace in execution order: the common case), anything else
//                                           four 4-byte loads. Heights below 4, and outputs or index lists that are not 16-byte
//                                           aligned, go word by word. Elements are addressed with 64 bits. The kernel writes every
//                                           word of the output, zero rows included.
// Direct mode (pw_apc_sources_from_traces_flags with PW_APC_SOURCES_DIRECT, pw_apc_sources_tracegen): no source matrix is
// built; the handle keeps the index lists of the place stage and the AIRs' trace pointers, and
//   tracegen   apc_sources_tracegen_kernel  out[apc_col * H + r] = r < n_calls ? trace_A[col * H_A + L[r * rbs + occ]] : 0, ONE launch for
//                                           all jobs: a workgroup is (job, instruction, tile of kTileRows rows, group of up to kColGroup of
//                                           the instruction's cells) and finds its item by binary search over the items' first tiles. A
//                                           lane owns 4 consecutive rows, reads its 4 list entries once (a strided read) and reuses them
//                                           over the group's cells; stores and loads as in the gather. Only the named columns are written.
#include "bus_shared.hpp"
#include "prover_internal.hpp"
#include "trace_entry.hpp"

#include <rocprim/rocprim.hpp>

#include <memory>

namespace pw {

namespace {

using namespace bus;

constexpr uint32_t kTileRows = 4 * kBlock;  // output rows of a workgroup: 4 per lane
constexpr uint32_t kColGroup = 16;          // columns of a workgroup

struct GatherJobDev {
    const uint32_t* in;
    const uint32_t* idx;
    uint32_t* out;
    u64 h_in, h_out, tile0;  // tile0: the job's first tile among all tiles of the launch
    uint32_t width, row_tiles, word, pad;
};

// counters: [0] tiles whose loads were all 16-byte loads (or none: zero rows) | [1] tiles with 4-byte loads
__global__ __launch_bounds__(kBlock) void apc_sources_gather_kernel(const GatherJobDev* __restrict__ jobs, uint32_t n_jobs, u64 tile_base, u64* __restrict__ counters) {
    const u64 t = tile_base + blockIdx.x;
    uint32_t lo = 0, hi = n_jobs;  // the last job with tile0 <= t
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (jobs[mid].tile0 <= t) lo = mid + 1;
        else hi = mid;
    }
    const GatherJobDev J = jobs[lo - 1];
    const u64 local = t - J.tile0;
    const u64 r0 = (local % J.row_tiles) * kTileRows + (u64)threadIdx.x * 4;
    const uint32_t c0 = (uint32_t)(local / J.row_tiles) * kColGroup, c1 = c0 + kColGroup < J.width ? c0 + kColGroup : J.width;
    bool words = false;
    if (J.word) {
        for (uint32_t k = 0; k < 4u && r0 + k < J.h_out; ++k) {
            const u64 r = r0 + k;
            const uint32_t s = J.idx[r];
            for (uint32_t c = c0; c < c1; ++c) J.out[(u64)c * J.h_out + r] = s < J.h_in ? J.in[(u64)c * J.h_in + s] : 0u;
            words = true;
        }
    } else if (r0 < J.h_out) {  // (h_out is a power of two >= 4 and r0 a multiple of 4: rows r0 .. r0 + 3 exist)
        const uint4 s = *reinterpret_cast<const uint4*>(J.idx + r0);
        uint32_t* __restrict__ out = J.out + r0;
        // (h_in is a power of two <= 2^31: s.x + 3 does not wrap, and with h_in >= 4 every column starts 16-byte aligned if `in` does)
        const bool run = s.x < J.h_in && s.y == s.x + 1u && s.z == s.x + 2u && s.w == s.x + 3u && s.w < J.h_in && ((((uintptr_t)J.in >> 2) + s.x) & 3u) == 0u;
        if (run) {
            const uint32_t* __restrict__ in = J.in + s.x;
#pragma unroll 4
            for (uint32_t c = c0; c < c1; ++c) *reinterpret_cast<uint4*>(out + (u64)c * J.h_out) = *reinterpret_cast<const uint4*>(in + (u64)c * J.h_in);
        } else if (s.x >= J.h_in && s.y >= J.h_in && s.z >= J.h_in && s.w >= J.h_in) {
            for (uint32_t c = c0; c < c1; ++c) *reinterpret_cast<uint4*>(out + (u64)c * J.h_out) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            words = true;
#pragma unroll 4
            for (uint32_t c = c0; c < c1; ++c) {
                const uint32_t* __restrict__ in = J.in + (u64)c * J.h_in;
                uint4 v;
                v.x = s.x < J.h_in ? in[s.x] : 0u;
                v.y = s.y < J.h_in ? in[s.y] : 0u;
                v.z = s.z < J.h_in ? in[s.z] : 0u;
                v.w = s.w < J.h_in ? in[s.w] : 0u;
                *reinterpret_cast<uint4*>(out + (u64)c * J.h_out) = v;
            }
        }
    }
    const int any_words = __syncthreads_or(words);
    if (threadIdx.x == 0u) atomicAdd(counters + (any_words ? 1 : 0), 1ull);
}

struct TraceItemDev {
    const uint32_t* in;    // the trace of the instruction's AIR (NULL with h_in = 0: an APC without calls)
    const uint32_t* list;  // the index list of (APC, AIR) from occ on: call r reads list[r * rbs]
    uint32_t* out;
    u64 h_in, h_out, n_calls, tile0;  // tile0: the item's first tile among all tiles of the launch
    uint32_t rbs, cell0, n_cells, word;  // cells cell0 .. cell0 + n_cells - 1 of the cell table: (col, apc_col)
};

// counters: as apc_sources_gather_kernel's
__global__ __launch_bounds__(kBlock) void apc_sources_tracegen_kernel(const TraceItemDev* __restrict__ items, uint32_t n_items, const uint2* __restrict__ cells,
                                                                       u64 tile_base, u64* __restrict__ counters) {
    const u64 t = tile_base + blockIdx.x;
    uint32_t lo = 0, hi = n_items;  // the last item with tile0 <= t
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (items[mid].tile0 <= t) lo = mid + 1;
        else hi = mid;
    }
    const TraceItemDev I = items[lo - 1];
    const u64 r0 = (t - I.tile0) * kTileRows + (u64)threadIdx.x * 4;
    const uint2* __restrict__ cell = cells + I.cell0;
    bool words = false;
    if (I.word) {
        for (uint32_t k = 0; k < 4u && r0 + k < I.h_out; ++k) {
            const u64 r = r0 + k;
            const uint32_t s = r < I.n_calls ? I.list[r * I.rbs] : ~0u;
            for (uint32_t c = 0; c < I.n_cells; ++c) I.out[(u64)cell[c].y * I.h_out + r] = s < I.h_in ? I.in[(u64)cell[c].x * I.h_in + s] : 0u;
            words = true;
        }
    } else if (r0 < I.h_out) {  // (h_out is a power of two >= 4 and r0 a multiple of 4: rows r0 .. r0 + 3 exist)
        uint4 s;
        s.x = r0 < I.n_calls ? I.list[r0 * I.rbs] : ~0u;
        s.y = r0 + 1 < I.n_calls ? I.list[(r0 + 1) * I.rbs] : ~0u;
        s.z = r0 + 2 < I.n_calls ? I.list[(r0 + 2) * I.rbs] : ~0u;
        s.w = r0 + 3 < I.n_calls ? I.list[(r0 + 3) * I.rbs] : ~0u;
        uint32_t* __restrict__ out = I.out + r0;
        // (h_in is a power of two <= 2^31: s.x + 3 does not wrap, and with h_in >= 4 every column starts 16-byte aligned if `in` does)
        const bool run = s.x < I.h_in && s.y == s.x + 1u && s.z == s.x + 2u && s.w == s.x + 3u && s.w < I.h_in && ((((uintptr_t)I.in >> 2) + s.x) & 3u) == 0u;
        if (run) {
            const uint32_t* __restrict__ in = I.in + s.x;
#pragma unroll 4
            for (uint32_t c = 0; c < I.n_cells; ++c) *reinterpret_cast<uint4*>(out + (u64)cell[c].y * I.h_out) = *reinterpret_cast<const uint4*>(in + (u64)cell[c].x * I.h_in);
        } else if (s.x >= I.h_in && s.y >= I.h_in && s.z >= I.h_in && s.w >= I.h_in) {
            for (uint32_t c = 0; c < I.n_cells; ++c) *reinterpret_cast<uint4*>(out + (u64)cell[c].y * I.h_out) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            words = true;
#pragma unroll 4
            for (uint32_t c = 0; c < I.n_cells; ++c) {
                const uint32_t* __restrict__ in = I.in + (u64)cell[c].x * I.h_in;
                uint4 v;
                v.x = s.x < I.h_in ? in[s.x] : 0u;
                v.y = s.y < I.h_in ? in[s.y] : 0u;
                v.z = s.z < I.h_in ? in[s.z] : 0u;
                v.w = s.w < I.h_in ? in[s.w] : 0u;
                *reinterpret_cast<uint4*>(out + (u64)cell[c].y * I.h_out) = v;
            }
        }
    }
    const int any_words = __syncthreads_or(words);
    if (threadIdx.x == 0u) atomicAdd(counters + (any_words ? 1 : 0), 1ull);
}

// what the place kernels read: the positions' global rows, the calls, the APCs with calls, the parts' first global rows
struct PlaceTables {
    const uint32_t* idx_s;   // global row of position i
    const u64* cov_off;      // [n_calls + 1] covered positions before call j
    const u64* from;         // [n_calls]
    const uint32_t* apc;     // [n_calls]
    const uint32_t* rank;    // [n_calls] the call's index among the calls of its APC
    const u64* first_from;   // [n_apcs] where the APC's first call starts
    const uint32_t* ioff;    // [n_apcs] the APC's first entry in the per-instruction arrays
    const u64* part_g0;      // [n_parts + 1]
    uint32_t n_calls, n_parts;
};

__device__ __forceinline__ uint32_t call_of(const PlaceTables& t, u64 c) {
    uint32_t lo = 0, hi = t.n_calls;  // the last call with cov_off <= c
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.cov_off[mid] <= c) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

__device__ __forceinline__ uint32_t part_of(const PlaceTables& t, u64 g) {
    uint32_t lo = 0, hi = t.n_parts;  // the last part with g0 <= g
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (t.part_g0[mid] <= g) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// c = a covered position counted through the calls; bad: the smallest position whose AIR is not the first call's
__global__ __launch_bounds__(kBlock) void apc_sources_layout_kernel(PlaceTables t, u64 n_covered, uint32_t* __restrict__ air_of, u64* __restrict__ bad) {
    const u64 c = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_covered) return;
    const uint32_t j = call_of(t, c), a = t.apc[j];
    const u64 k = c - t.cov_off[j], pos = t.from[j] + k, first = t.first_from[a];
    const uint32_t part = part_of(t, t.idx_s[pos]);
    if (t.from[j] == first) air_of[t.ioff[a] + k] = part;
    else if (part_of(t, t.idx_s[first + k]) != part) atomicMin(bad, pos);
}

// after the layout stands (every call of an APC has the first call's AIRs): the index lists of the sources and the covered flags
__global__ __launch_bounds__(kBlock) void apc_sources_place_kernel(PlaceTables t, u64 n_covered, const uint32_t* __restrict__ air_of, const uint32_t* __restrict__ occ,
                                                                    const u64* __restrict__ list_base, const uint32_t* __restrict__ rbs, uint32_t* __restrict__ lists,
                                                                    uint8_t* __restrict__ covered) {
    const u64 c = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_covered) return;
    const uint32_t j = call_of(t, c), a = t.apc[j];
    const u64 k = c - t.cov_off[j], g = t.idx_s[t.from[j] + k], i = t.ioff[a] + k;
    const uint32_t part = air_of[i];
    const u64 pair = (u64)a * t.n_parts + part;
    lists[list_base[pair] + (u64)t.rank[j] * rbs[pair] + occ[i]] = (uint32_t)(g - t.part_g0[part]);
    covered[g] = 1;
}

// covered[g] becomes keep[g]: an active row no call covers
__global__ __launch_bounds__(kBlock) void apc_sources_keep_kernel(const u64* __restrict__ tkey, uint8_t* __restrict__ covered, u64 M) {
    const u64 g = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (g < M) covered[g] = tkey[g] != kEmpty && !covered[g];
}

struct AsU32 {
    __device__ uint32_t operator()(uint8_t f) const { return f; }
};

// starts[p] = kept rows before part p's first row; starts[n_parts] = all kept rows
__global__ void apc_sources_starts_kernel(const uint32_t* __restrict__ off, const uint8_t* __restrict__ keep, const u64* __restrict__ part_g0, uint32_t n_parts, u64 M,
                                          uint32_t* __restrict__ starts) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p < n_parts) starts[p] = off[part_g0[p]];
    else if (p == n_parts) starts[p] = off[M - 1] + keep[M - 1];
}

__global__ __launch_bounds__(kBlock) void apc_sources_residual_kernel(PlaceTables t, const uint8_t* __restrict__ keep, const uint32_t* __restrict__ off,
                                                                       const uint32_t* __restrict__ starts, const u64* __restrict__ list_base, u64 M,
                                                                       uint32_t* __restrict__ lists) {
    const u64 g = (u64)blockIdx.x * kBlock + threadIdx.x;
    if (g >= M || !keep[g]) return;
    const uint32_t part = part_of(t, g);
    lists[list_base[part] + (off[g] - starts[part])] = (uint32_t)(g - t.part_g0[part]);
}

struct AsCtx : Scratch {  // (its `extra`: the matrices of the handle under construction)
    time_index::Stage index{*this};
    Buf temp{*this}, small{*this}, small2{*this}, small3{*this}, lists{*this}, rlists{*this}, covered{*this}, off{*this}, jobs{*this};
    uint64_t stat_covered = 0, stat_source_bytes = 0, stat_residual_bytes = 0, stat_jobs = 0, stat_tiles16 = 0, stat_tiles4 = 0;
    void reset_stats() override { stat_covered = stat_source_bytes = stat_residual_bytes = stat_jobs = stat_tiles16 = stat_tiles4 = 0; }
};
thread_local AsCtx g_as;
struct TracegenStats {
    uint64_t jobs = 0, items = 0, tiles16 = 0, tiles4 = 0, bytes_written = 0;
};
thread_local TracegenStats g_tracegen;

bool power_of_two(u64 x) { return x && !(x & (x - 1)); }
u64 next_power_of_two(u64 x) {
    u64 p = 1;
    while (p < x) p <<= 1;
    return p;
}

// false = -1: a NULL pointer, a height that is no power of two (or a source of more than 2^31 rows, which no index reaches), no column
bool jobs_well_formed(const PwGatherJob* jobs, size_t n_jobs) {
    if (!jobs && n_jobs) return false;
    for (size_t k = 0; k < n_jobs; ++k) {
        const PwGatherJob& j = jobs[k];
        if (!j.in || !j.idx || !j.out || !power_of_two(j.h_in) || !power_of_two(j.h_out) || j.h_in > ((u64)1 << 31) || j.h_out > ((u64)1 << 32) || !j.width ||
            j.width >= ((u64)1 << 32))
            return false;
    }
    return true;
}

size_t job_table_bytes(size_t n_jobs) { return 64 + n_jobs * sizeof(GatherJobDev); }

// all jobs in one launch (more than 2^30 tiles: one launch per 2^30); the call returns after the stream has run them
int gather(AsCtx& cx, const PwGatherJob* jobs, size_t n_jobs) {
    if (!n_jobs) return 0;
    hipStream_t st = stream();
    std::vector<char> image(job_table_bytes(n_jobs), 0);  // two counters, then the job table
    GatherJobDev* tab = reinterpret_cast<GatherJobDev*>(image.data() + 64);
    u64 tiles = 0;
    for (size_t k = 0; k < n_jobs; ++k) {
        const PwGatherJob& j = jobs[k];
        const u64 row_tiles = (j.h_out + kTileRows - 1) / kTileRows, col_groups = (j.width + kColGroup - 1) / kColGroup;
        const bool word = j.h_out < 4 || (((uintptr_t)j.out | (uintptr_t)j.idx) & 15u) != 0;
        tab[k] = GatherJobDev{j.in, j.idx, j.out, j.h_in, j.h_out, tiles, (uint32_t)j.width, (uint32_t)row_tiles, word ? 1u : 0u, 0u};
        tiles += row_tiles * col_groups;
    }
    ScopedKernelTimer timer("apc_sources_gather");
    PW_TRY(cx.jobs.ensure(image.size()));
    PW_HIP_TRY(hipMemcpyAsync(cx.jobs.p, image.data(), image.size(), hipMemcpyHostToDevice, st));
    const u64 per_launch = (u64)1 << 30;
    for (u64 base = 0; base < tiles; base += per_launch)
        hipLaunchKernelGGL(apc_sources_gather_kernel, dim3((unsigned)std::min(per_launch, tiles - base)), dim3(kBlock), 0, st,
                           (const GatherJobDev*)(cx.jobs.as<char>() + 64), (uint32_t)n_jobs, base, cx.jobs.as<u64>());
    PW_HIP_TRY(hipGetLastError());
    u64 counters[2] = {0, 0};
    PW_HIP_TRY(hipMemcpyAsync(counters, cx.jobs.p, sizeof counters, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));  // (image and counters are locals)
    cx.stat_jobs = n_jobs;
    cx.stat_tiles16 = counters[0];
    cx.stat_tiles4 = counters[1];
    return 0;
}

// matrices laid out in one allocation, each 256-byte aligned
size_t place_matrix(size_t& total, size_t words) {
    const size_t at = (total + 255) & ~(size_t)255;
    total = at + words * 4;
    return at;
}

}  // namespace

}  // namespace pw

using namespace pw;

struct PwApcSources {
    struct Source { size_t at = 0; u64 height = 0; uint32_t width = 0, rbs = 0; };
    struct Residual { size_t at = 0; u64 rows = 0; uint32_t log_height = 0, width = 0; bool part = false; };
    DeviceBuf src, res;
    size_t n_apcs = 0, n_airs = 0;
    std::vector<Source> sources;      // [n_apcs x n_airs]
    std::vector<Residual> residuals;  // [n_airs]
    std::vector<uint64_t> n_calls;    // [n_apcs]
    std::vector<uint32_t> cycle, ioff, air_of, occ;  // per APC its cycle count and first entry; per instruction of an APC with calls (AIR, occ)
    uint64_t positions = 0, covered = 0, source_bytes = 0, residual_bytes = 0;
    // direct mode: no source matrix (height 0 everywhere); the index lists, where each (APC, AIR) pair's begins, the callers' traces
    struct Trace { const uint32_t* p = nullptr; u64 height = 0; uint32_t width = 0; };
    bool direct = false;
    DeviceBuf idx;
    std::vector<u64> list_base;  // [n_apcs x n_airs] in words
    std::vector<Trace> traces;   // [n_airs], set for the AIRs that take part
};

extern "C" void pw_apc_sources_destroy(PwApcSources* e) { delete e; }

extern "C" void pw_apc_sources_sizes(const PwApcSources* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->n_apcs;
    sizes[1] = e->n_airs;
    sizes[2] = e->positions;
    sizes[3] = e->covered;
    sizes[4] = e->source_bytes;
    sizes[5] = e->residual_bytes;
}

extern "C" int64_t pw_apc_sources_layout(const PwApcSources* e, uint32_t apc, uint64_t* n_calls, uint32_t* air, uint32_t* occ) {
    if (!e || apc >= e->n_apcs) return -1;
    if (n_calls) *n_calls = e->n_calls[apc];
    if (!e->n_calls[apc]) return 0;
    const uint32_t L = e->cycle[apc], at = e->ioff[apc];
    if (air) std::copy(e->air_of.begin() + at, e->air_of.begin() + at + L, air);
    if (occ) std::copy(e->occ.begin() + at, e->occ.begin() + at + L, occ);
    return L;
}

extern "C" int pw_apc_sources_source(const PwApcSources* e, uint32_t apc, uint32_t air, const uint32_t** d_matrix, uint32_t* width, uint64_t* height,
                                     uint32_t* row_block_size) {
    if (!e || apc >= e->n_apcs || air >= e->n_airs) return -1;
    const PwApcSources::Source& s = e->sources[(size_t)apc * e->n_airs + air];
    if (d_matrix) *d_matrix = s.height ? (const uint32_t*)((const char*)e->src.p + s.at) : nullptr;
    if (width) *width = s.width;
    if (height) *height = s.height;
    if (row_block_size) *row_block_size = s.rbs;
    return 0;
}

extern "C" int pw_apc_sources_residual(const PwApcSources* e, uint32_t air, const uint32_t** d_matrix, uint64_t* rows, uint32_t* log_height) {
    if (!e || air >= e->n_airs) return -1;
    const PwApcSources::Residual& r = e->residuals[air];
    if (d_matrix) *d_matrix = r.part ? (const uint32_t*)((const char*)e->res.p + r.at) : nullptr;
    if (rows) *rows = r.rows;
    if (log_height) *log_height = r.log_height;
    return r.part ? 1 : 0;
}

extern "C" int pw_apc_sources_read_source(const PwApcSources* e, uint32_t apc, uint32_t air, uint32_t* words) {
    if (!e || apc >= e->n_apcs || air >= e->n_airs || !words) return -1;
    const PwApcSources::Source& s = e->sources[(size_t)apc * e->n_airs + air];
    if (!s.height) return 0;
    PW_HIP_TRY(hipMemcpyAsync(words, (const char*)e->src.p + s.at, (size_t)s.width * s.height * 4, hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

extern "C" int pw_apc_sources_read_residual(const PwApcSources* e, uint32_t air, uint32_t* words) {
    if (!e || air >= e->n_airs || !words) return -1;
    const PwApcSources::Residual& r = e->residuals[air];
    if (!r.part) return 0;
    PW_HIP_TRY(hipMemcpyAsync(words, (const char*)e->res.p + r.at, ((size_t)r.width << r.log_height) * 4, hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

extern "C" void pw_apc_sources_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_as.stat_covered;
    out[1] = g_as.stat_source_bytes;
    out[2] = g_as.stat_residual_bytes;
    out[3] = g_as.stat_jobs;
    out[4] = g_as.stat_tiles16;
    out[5] = g_as.stat_tiles4;
    out[6] = g_as.peak();
    out[7] = g_as.held();
}

extern "C" uint64_t pw_apc_sources_index_bytes(const PwApcSources* e) { return e ? e->idx.bytes : 0; }

extern "C" void pw_apc_sources_tracegen_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_tracegen.jobs;
    out[1] = g_tracegen.items;
    out[2] = g_tracegen.tiles16;
    out[3] = g_tracegen.tiles4;
    out[4] = g_tracegen.bytes_written;
    out[5] = g_as.held();
}

extern "C" int pw_apc_sources_tracegen(const PwApcSources* e, const PwApcTraceJob* jobs, size_t n_jobs) {
    if (!e || !e->direct || (!jobs && n_jobs) || n_jobs >= ((size_t)1 << 31)) return -1;
    // ---- every refusal, and the tables (host): per job its cells by (instr, col), an item per instruction and group of kColGroup cells ----
    std::vector<TraceItemDev> items;
    std::vector<uint2> cells;
    std::vector<std::pair<uintptr_t, uintptr_t>> spans;  // the jobs' output matrices [begin, end)
    std::vector<PwApcCell> sorted;
    std::vector<uint32_t> apc_cols;
    u64 tiles = 0, bytes_written = 0;
    for (size_t k = 0; k < n_jobs; ++k) {
        const PwApcTraceJob& j = jobs[k];
        if ((!j.cells && j.n_cells) || !j.d_out || j.apc >= e->n_apcs || !j.out_width || !power_of_two(j.out_height) || j.out_height > ((u64)1 << 32) ||
            j.out_height < e->n_calls[j.apc] || j.n_cells >= ((size_t)1 << 32))
            return -1;
        const uint32_t apc = j.apc, cycle = e->cycle[apc], at = e->ioff[apc];
        const u64 n_calls = e->n_calls[apc];
        sorted.assign(j.cells, j.cells + j.n_cells);
        apc_cols.resize(j.n_cells);
        for (size_t c = 0; c < j.n_cells; ++c) {
            const PwApcCell& x = sorted[c];
            if (x.instr >= cycle || x.apc_col >= j.out_width || (n_calls && x.col >= e->traces[e->air_of[at + x.instr]].width)) return -1;
            apc_cols[c] = x.apc_col;
        }
        std::sort(apc_cols.begin(), apc_cols.end());
        if (std::adjacent_find(apc_cols.begin(), apc_cols.end()) != apc_cols.end()) return -1;
        std::sort(sorted.begin(), sorted.end(), [](const PwApcCell& a, const PwApcCell& b) {
            return a.instr != b.instr ? a.instr < b.instr : a.col != b.col ? a.col < b.col : a.apc_col < b.apc_col;
        });
        const uintptr_t begin = (uintptr_t)j.d_out;
        spans.emplace_back(begin, begin + (uintptr_t)j.out_width * j.out_height * 4);
        const u64 row_tiles = (j.out_height + kTileRows - 1) / kTileRows;
        const uint32_t word = j.out_height < 4 || (begin & 15u) != 0 ? 1u : 0u;
        for (size_t c = 0; c < j.n_cells;) {
            size_t c1 = c;
            while (c1 < j.n_cells && c1 - c < kColGroup && sorted[c1].instr == sorted[c].instr) ++c1;
            TraceItemDev it{nullptr, nullptr, j.d_out, 0, j.out_height, n_calls, tiles, 1u, (uint32_t)cells.size(), (uint32_t)(c1 - c), word};
            if (n_calls) {
                const uint32_t air = e->air_of[at + sorted[c].instr];
                const PwApcSources::Source& s = e->sources[(size_t)apc * e->n_airs + air];
                it.in = e->traces[air].p;
                it.h_in = e->traces[air].height;
                it.list = (const uint32_t*)e->idx.p + e->list_base[(size_t)apc * e->n_airs + air] + e->occ[at + sorted[c].instr];
                it.rbs = s.rbs;
            }
            items.push_back(it);
            for (; c < c1; ++c) cells.push_back(make_uint2(sorted[c].col, sorted[c].apc_col));
            tiles += row_tiles;
        }
        bytes_written += (u64)j.n_cells * j.out_height * 4;
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k].first < spans[k - 1].second) return -1;
    if (cells.size() >= ((size_t)1 << 32) || items.size() >= ((size_t)1 << 31)) return -1;
    g_tracegen = TracegenStats{};
    g_tracegen.jobs = n_jobs;
    g_tracegen.items = items.size();
    if (items.empty()) return 0;

    // ---- one launch (more than 2^30 tiles: one launch per 2^30); the call returns after the stream has run it ----
    AsCtx& cx = g_as;
    const ScratchCall call(cx, ScratchCall::kContinues);
    hipStream_t st = stream();
    Image im;
    const size_t at_counters = im.put(std::vector<u64>(8, 0)), at_items = im.put(items), at_cells = im.put(cells);
    if (im.bytes.size() + 16 > call.bound(0)) return (int)hipErrorOutOfMemory;
    ScopedKernelTimer timer("apc_sources_tracegen");
    PW_TRY(im.upload(cx.jobs, st));
    char* tab = cx.jobs.as<char>();
    const u64 per_launch = (u64)1 << 30;
    for (u64 base = 0; base < tiles; base += per_launch)
        hipLaunchKernelGGL(apc_sources_tracegen_kernel, dim3((unsigned)std::min(per_launch, tiles - base)), dim3(kBlock), 0, st, (const TraceItemDev*)(tab + at_items),
                           (uint32_t)items.size(), (const uint2*)(tab + at_cells), base, (u64*)(tab + at_counters));
    PW_HIP_TRY(hipGetLastError());
    u64 counters[2] = {0, 0};
    PW_HIP_TRY(hipMemcpyAsync(counters, tab + at_counters, sizeof counters, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));  // (the image and counters are locals)
    g_tracegen.tiles16 = counters[0];
    g_tracegen.tiles4 = counters[1];
    g_tracegen.bytes_written = bytes_written;
    return 0;
}

extern "C" int pw_trace_gather_rows(const PwGatherJob* jobs, size_t n_jobs) {
    if (!jobs_well_formed(jobs, n_jobs)) return -1;
    AsCtx& cx = g_as;
    const ScratchCall call(cx);
    return gather(cx, jobs, n_jobs);
}

extern "C" int pw_apc_sources_from_traces_flags(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, const uint32_t* cycle_counts,
                                                size_t n_apcs, const uint32_t* call_apc_ids, const uint64_t* call_from, const uint64_t* call_to, size_t n_calls,
                                                uint32_t min_log_height, size_t scratch_bytes, uint32_t flags, PwApcSources** out, uint32_t* status, uint64_t* info) {
    if ((flags & ~PW_APC_SOURCES_DIRECT) || !out || !status || !info || bridge_bus >= bb::P || min_log_height > 31u || !time_index::one_segment(segment_of_air, n_airs) ||
        !time_index::calls_well_formed(cycle_counts, n_apcs, call_apc_ids, call_from, call_to, n_calls))
        return -1;
    time_index::Bridge B;
    if (!airs_well_formed(airs, n_airs) || !time_index::bridge_of(airs, n_airs, bridge_bus, &B) || B.M + 1 >= ((u64)1 << 32)) return -1;
    const u64 M = B.M, min_h = (u64)1 << min_log_height;
    const bool direct = (flags & PW_APC_SOURCES_DIRECT) != 0;
    AsCtx& cx = g_as;
    const ScratchCall call(cx, out, status, info);

    // ---- the calls, per APC (host) ----
    std::vector<u64> cov_off(n_calls + 1, 0), first_from(n_apcs, 0), calls_of(n_apcs, 0);
    std::vector<uint32_t> rank(n_calls, 0), ioff(n_apcs, 0);
    for (size_t j = 0; j < n_calls; ++j) {
        const uint32_t a = call_apc_ids[j];
        cov_off[j + 1] = cov_off[j] + cycle_counts[a];
        if (!calls_of[a]) first_from[a] = call_from[j];
        rank[j] = (uint32_t)calls_of[a]++;
    }
    const u64 n_covered = cov_off[n_calls];
    u64 n_instr = 0;  // the instructions of the APCs that have calls
    for (size_t a = 0; a < n_apcs; ++a)
        if (calls_of[a]) {
            ioff[a] = (uint32_t)n_instr;
            n_instr += cycle_counts[a];
        }

    // ---- the AIRs that take part: those with the bridge ----
    const std::vector<size_t>& part_air = B.part_air;
    const std::vector<u64>& g0 = B.g0;
    const size_t n_parts = B.n_parts();

    // ---- status 2: what is known before a row is read ----
    const size_t bound = call.bound(scratch_bytes);
    {
        // per APC with n calls of L instructions: its rows in an AIR are distinct rows of that AIR, and over all AIRs n * L rows
        // (a power of two at most doubles them); the residual of an AIR is at most the AIR. Direct mode has no source matrices, and its
        // lists are not padded to a matrix's height: n * L entries per APC
        size_t out_bytes = 0, list_rows = 0, width_max = 0, floor_bytes = 0;
        for (size_t k = 0; k < n_parts; ++k) {
            const size_t w = airs[part_air[k]].prover->width, h = std::max<u64>(min_h, (u64)1 << airs[part_air[k]].log_height);
            width_max = std::max(width_max, w);
            floor_bytes += w * 4 * min_h;
            out_bytes += w * 4 * h;
            list_rows += h;
        }
        for (size_t a = 0; a < n_apcs; ++a) {
            if (!calls_of[a]) continue;
            const u64 cover = calls_of[a] * cycle_counts[a], cover2 = next_power_of_two(cover);
            if (direct) {
                list_rows += cover;
                continue;
            }
            size_t by_air = 0, rows_by_air = 0;
            for (size_t k = 0; k < n_parts; ++k) {
                const u64 h = std::max<u64>(min_h, std::min<u64>(cover2, (u64)1 << airs[part_air[k]].log_height));
                by_air += (size_t)airs[part_air[k]].prover->width * 4 * h;
                rows_by_air += h;
            }
            out_bytes += std::min<size_t>(by_air, 2 * cover * width_max * 4 + floor_bytes);
            list_rows += std::min<size_t>(rows_by_air, 2 * cover + n_parts * min_h);
        }
        const size_t n_lists = (n_apcs + 1) * n_parts;
        const size_t tables = 4096 + n_calls * 32 + n_apcs * 32 + n_instr * 8 + n_lists * 32 + job_table_bytes(n_lists) + 256 * (n_lists + 2);
        const size_t index_need = time_index::bytes_needed(M);
        const size_t place_need = 64 + (size_t)M * 17 + (M ? time_index::scan_temp(rocprim::make_transform_iterator((const uint8_t*)nullptr, AsU32{}), M) : 0);
        const size_t need = ((size_t)1 << 20) + tables + std::max(index_need, place_need) + out_bytes + (list_rows + 4 * n_lists) * 4;
        if (bound < need) {
            *status = 2;
            *info = need;
            return 0;
        }
    }

    auto result = std::make_unique<PwApcSources>();
    PwApcSources& R = *result;
    R.n_apcs = n_apcs;
    R.n_airs = n_airs;
    R.direct = direct;
    R.traces.resize(n_airs);
    R.list_base.assign(direct ? n_apcs * n_airs : 0, 0);
    R.sources.resize(n_apcs * n_airs);
    R.residuals.resize(n_airs);
    R.n_calls.assign(calls_of.begin(), calls_of.end());
    R.cycle.assign(cycle_counts, cycle_counts + n_apcs);
    R.ioff = ioff;
    R.covered = n_covered;
    cx.stat_covered = n_covered;

    // ---- index ----
    hipStream_t st = stream();
    u64 N = 0;
    PW_TRY(time_index::open(airs, segment_of_air, n_airs, bridge_bus, B, cx.index, cx.temp,
                            time_index::Names{"apc_sources_index_kernel", "apc_sources_sort_time", "apc_sources_time_kernel"}, &N, status, info));
    if (*status) return (int)hipGetLastError();
    cx.index.release_except({&cx.index.tkey, &cx.index.idx_s});  // the keys say which rows are active, the order places the calls
    cx.temp.release();
    R.positions = N;
    if (!time_index::calls_within(call_to, n_calls, N, status, info)) return 0;
    if (!M) {  // no AIR takes part (and so no call): nothing to build
        *out = result.release();
        return 0;
    }

    // ---- place ----
    const dim3 block(kBlock);
    PlaceTables T{};
    std::vector<uint32_t> air_of(n_instr, 0), occ(n_instr, 0), rbs(n_apcs * n_parts, 0);
    std::vector<u64> list_base(n_apcs * n_parts, 0);
    size_t src_total = 0;
    {
        ScopedKernelTimer timer("apc_sources_place");
        Image im;
        const std::vector<u64> bad0{kEmpty};
        const size_t at_bad = im.put(bad0), at_cov = im.put(cov_off), at_from = im.put(std::vector<u64>(call_from, call_from + n_calls)),
                     at_apc = im.put(std::vector<uint32_t>(call_apc_ids, call_apc_ids + n_calls)), at_rank = im.put(rank), at_first = im.put(first_from),
                     at_ioff = im.put(ioff), at_g0 = im.put(g0), at_air = im.put(air_of);
        PW_TRY(im.upload(cx.small, st));
        char* sm = cx.small.as<char>();
        T = PlaceTables{(const uint32_t*)cx.index.idx_s.p, (const u64*)(sm + at_cov), (const u64*)(sm + at_from), (const uint32_t*)(sm + at_apc), (const uint32_t*)(sm + at_rank),
                        (const u64*)(sm + at_first), (const uint32_t*)(sm + at_ioff), (const u64*)(sm + at_g0), (uint32_t)n_calls, (uint32_t)n_parts};
        uint32_t* d_air_of = (uint32_t*)(sm + at_air);
        if (n_covered) {
            hipLaunchKernelGGL(apc_sources_layout_kernel, dim3(div_up(n_covered, kBlock)), block, 0, st, T, n_covered, d_air_of, (u64*)(sm + at_bad));
            PW_HIP_TRY(hipGetLastError());
        }
        u64 bad = kEmpty;
        PW_HIP_TRY(hipMemcpyAsync(&bad, sm + at_bad, 8, hipMemcpyDeviceToHost, st));
        if (n_instr) PW_HIP_TRY(hipMemcpyAsync(air_of.data(), d_air_of, n_instr * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        if (bad != kEmpty) {
            *status = 12;
            *info = bad;
            return 0;
        }
        // occ and rbs: a pass over the instructions of the APCs with calls; then the source matrices and their index lists
        size_t list_total = 0;
        for (size_t a = 0; a < n_apcs; ++a) {
            if (!calls_of[a]) continue;
            uint32_t* per_part = rbs.data() + a * n_parts;
            for (uint32_t k = 0; k < cycle_counts[a]; ++k) occ[ioff[a] + k] = per_part[air_of[ioff[a] + k]]++;
            for (size_t k = 0; k < n_parts; ++k) {
                if (!per_part[k]) continue;
                const size_t air = part_air[k];
                PwApcSources::Source& s = R.sources[a * n_airs + air];
                s.width = airs[air].prover->width;
                s.rbs = per_part[k];
                list_base[a * n_parts + k] = list_total;
                if (direct) {  // (height stays 0: no matrix)
                    R.list_base[a * n_airs + air] = list_total;
                    R.traces[air] = PwApcSources::Trace{airs[air].d_trace, (u64)1 << airs[air].log_height, s.width};
                    list_total += (calls_of[a] * per_part[k] + 3) & ~(u64)3;
                    continue;
                }
                s.height = std::max<u64>(min_h, next_power_of_two(calls_of[a] * per_part[k]));
                s.at = place_matrix(src_total, (size_t)s.width * s.height);
                list_total += (s.height + 3) & ~(u64)3;
                R.source_bytes += (u64)s.width * s.height * 4;
            }
        }
        for (size_t i = 0; i < n_instr; ++i) air_of[i] = (uint32_t)part_air[air_of[i]];  // (the handle names AIRs, the device parts)
        R.air_of = air_of;
        R.occ = occ;
        PW_TRY(cx.covered.ensure(M));
        DeviceBuf& lists = direct ? R.idx : cx.lists;  // direct: the handle keeps them
        PW_TRY(lists.ensure(std::max<size_t>(list_total * 4, 16)));
        if (src_total) PW_TRY(R.src.ensure(src_total));
        cx.set_extra(R.src.bytes + R.idx.bytes);
        PW_HIP_TRY(hipMemsetAsync(cx.covered.p, 0, M, st));
        PW_HIP_TRY(hipMemsetAsync(lists.p, 0xff, std::max<size_t>(list_total * 4, 16), st));
        if (n_covered) {
            Image im2;
            const size_t at_occ = im2.put(occ), at_base = im2.put(list_base), at_rbs = im2.put(rbs);
            PW_TRY(im2.upload(cx.small2, st));
            char* s2 = cx.small2.as<char>();
            hipLaunchKernelGGL(apc_sources_place_kernel, dim3(div_up(n_covered, kBlock)), block, 0, st, T, n_covered, (const uint32_t*)d_air_of, (const uint32_t*)(s2 + at_occ),
                               (const u64*)(s2 + at_base), (const uint32_t*)(s2 + at_rbs), lists.as<uint32_t>(), cx.covered.as<uint8_t>());
            PW_HIP_TRY(hipGetLastError());
            PW_HIP_TRY(hipStreamSynchronize(st));  // (im2 is a local)
        }
    }

    // ---- residuals ----
    std::vector<u64> rlist_base(n_parts, 0);
    {
        ScopedKernelTimer timer("apc_sources_residual");
        PW_TRY(cx.off.ensure(M * 4));
        PW_TRY(cx.small3.ensure((n_parts + 1) * 4 + n_parts * 8 + 64));
        uint8_t* keep = cx.covered.as<uint8_t>();
        hipLaunchKernelGGL(apc_sources_keep_kernel, dim3(div_up(M, kBlock)), block, 0, st, (const u64*)cx.index.tkey.p, keep, M);
        PW_HIP_TRY(hipGetLastError());
        PW_TRY(with_temp(cx.temp, [&](void* t, size_t& b) {
            return rocprim::exclusive_scan(t, b, rocprim::make_transform_iterator((const uint8_t*)keep, AsU32{}), cx.off.as<uint32_t>(), 0u, (size_t)M,
                                           rocprim::plus<uint32_t>(), st);
        }));
        uint32_t* d_starts = cx.small3.as<uint32_t>();
        u64* d_rbase = (u64*)(cx.small3.as<char>() + (((n_parts + 1) * 4 + 15) & ~(size_t)15));
        hipLaunchKernelGGL(apc_sources_starts_kernel, dim3(div_up(n_parts + 1, 64)), dim3(64), 0, st, (const uint32_t*)cx.off.p, (const uint8_t*)keep, T.part_g0,
                           (uint32_t)n_parts, M, d_starts);
        PW_HIP_TRY(hipGetLastError());
        std::vector<uint32_t> starts(n_parts + 1, 0);
        PW_HIP_TRY(hipMemcpyAsync(starts.data(), d_starts, (n_parts + 1) * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        cx.index.tkey.release();
        size_t res_total = 0, rlist_total = 0;
        for (size_t k = 0; k < n_parts; ++k) {
            const size_t air = part_air[k];
            PwApcSources::Residual& r = R.residuals[air];
            r.part = true;
            r.width = airs[air].prover->width;
            r.rows = starts[k + 1] - starts[k];
            const u64 h = std::max<u64>(min_h, next_power_of_two(r.rows));
            while (((u64)1 << r.log_height) < h) ++r.log_height;
            r.at = place_matrix(res_total, (size_t)r.width * h);
            rlist_base[k] = rlist_total;
            rlist_total += (h + 3) & ~(u64)3;
            R.residual_bytes += (u64)r.width * h * 4;
        }
        PW_TRY(cx.rlists.ensure(std::max<size_t>(rlist_total * 4, 16)));
        PW_TRY(R.res.ensure(std::max<size_t>(res_total, 16)));
        cx.set_extra(R.src.bytes + R.idx.bytes + R.res.bytes);
        PW_HIP_TRY(hipMemsetAsync(cx.rlists.p, 0xff, std::max<size_t>(rlist_total * 4, 16), st));
        PW_HIP_TRY(hipMemcpyAsync(d_rbase, rlist_base.data(), n_parts * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(apc_sources_residual_kernel, dim3(div_up(M, kBlock)), block, 0, st, T, (const uint8_t*)keep, (const uint32_t*)cx.off.p, (const uint32_t*)d_starts,
                           (const u64*)d_rbase, M, cx.rlists.as<uint32_t>());
        PW_HIP_TRY(hipGetLastError());
        PW_HIP_TRY(hipStreamSynchronize(st));  // (rlist_base is a local)
    }
    for (Scratch::Buf* b : {&cx.covered, &cx.off, &cx.temp, &cx.index.idx_s, &cx.small, &cx.small2, &cx.small3}) b->release();

    // ---- gather: every source and every residual in one launch ----
    std::vector<PwGatherJob> jobs;
    for (size_t a = 0; a < n_apcs; ++a)
        for (size_t k = 0; k < n_parts; ++k) {
            const size_t air = part_air[k];
            const PwApcSources::Source& s = R.sources[a * n_airs + air];
            if (!s.height) continue;
            jobs.push_back(PwGatherJob{airs[air].d_trace, (u64)1 << airs[air].log_height, s.width, cx.lists.as<uint32_t>() + list_base[a * n_parts + k],
                                       (uint32_t*)(R.src.as<char>() + s.at), s.height});
        }
    for (size_t k = 0; k < n_parts; ++k) {
        const size_t air = part_air[k];
        const PwApcSources::Residual& r = R.residuals[air];
        jobs.push_back(PwGatherJob{airs[air].d_trace, (u64)1 << airs[air].log_height, r.width, cx.rlists.as<uint32_t>() + rlist_base[k], (uint32_t*)(R.res.as<char>() + r.at),
                                   (u64)1 << r.log_height});
    }
    PW_TRY(gather(cx, jobs.data(), jobs.size()));
    cx.stat_source_bytes = R.source_bytes;
    cx.stat_residual_bytes = R.residual_bytes;
    *out = result.release();
    return 0;
}

extern "C" int pw_apc_sources_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, const uint32_t* cycle_counts,
                                          size_t n_apcs, const uint32_t* call_apc_ids, const uint64_t* call_from, const uint64_t* call_to, size_t n_calls,
                                          uint32_t min_log_height, size_t scratch_bytes, PwApcSources** out, uint32_t* status, uint64_t* info) {
    return pw_apc_sources_from_traces_flags(airs, segment_of_air, n_airs, bridge_bus, cycle_counts, n_apcs, call_apc_ids, call_from, call_to, n_calls, min_log_height,
                                            scratch_bytes, 0, out, status, info);
}
