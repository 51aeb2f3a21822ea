// _apc_apply_derived_expr and _apc_apply_bus for gfx950.
//
// Reference semantics:
//   derived columns  /root/reference/openvm/cuda/src/apc_tracegen.cu:72-124
//                    (CPU twin: openvm/src/powdr_extension/trace_generator/cpu/mod.rs:182-202)
//   bus -> histogram /root/reference/openvm/cuda/src/apc_apply_bus.cu:23-169
//                    (CPU twin: .../cpu/periphery.rs:176-237)
//
// One lane per APC row; the bytecode is wave-uniform (see expr_eval.hpp).
// Differences from the reference launch, none of them observable in the result:
//   * interactions whose bus id is none of the three periphery buses are
//     skipped before their multiplicity is evaluated (the reference evaluates
//     it and then ignores it, apc_apply_bus.cu:58-63,111);
//   * a multiplicity m is applied as one atomicAdd(bin, m) instead of m single
//     increments (apc_apply_bus.cu:77,91,106) — same sum mod 2^32;
//   * the interaction list is additionally split over blockIdx.y so that short
//     traces still fill 256 CUs (histogram sums are order independent).
// Defined behaviour where the reference traps or writes out of bounds: a
// histogram index >= the bin count is dropped (index arithmetic is the
// reference's 32-bit wrap-around arithmetic); bitwise operands >= 256 or a
// selector other than 0/1 are ignored (reference: assert(false),
// apc_apply_bus.cu:109).
#include "babybear.hpp"
#include "common.hpp"
#include "expr_eval.hpp"
#include "xbc.hpp"
#include "xbc_compile.hpp"
#include "small_form.hpp"
#include "plan_cache.hpp"
#include "../../include/powdr_gpu.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

constexpr int kBlock = 256;

// col_stride = 1: PUSH_APC operands are element offsets col*H (reference encoding); col_stride = H: operands are
// column indices (extension for traces with W*H >= 2^32, which the u32 offsets cannot address).
__global__ __launch_bounds__(kBlock) void apc_apply_derived_expr_kernel(
    uint32_t* d_output, size_t H, int num_calls, const DerivedExprSpec* __restrict__ specs,
    size_t n_cols, const uint32_t* __restrict__ bytecode, size_t col_stride) {
    __shared__ uint32_t stack_lds[pw::kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t total = (size_t)gridDim.x * kBlock;
    for (size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x; r < H; r += total) {
        if (r < (size_t)num_calls) {
            for (size_t i = 0; i < n_cols; ++i) {
                const DerivedExprSpec spec = specs[i];
                // later derived columns may read earlier ones of the same row: plain
                // (non-restrict) accesses by the same thread keep program order.
                uint32_t v = pw::eval_expr<kBlock, true>(bytecode + spec.span.off, spec.span.len,
                                                        d_output, r, stk, col_stride);
                d_output[spec.col_base + r] = v;
            }
        } else {
            for (size_t i = 0; i < n_cols; ++i) d_output[specs[i].col_base + r] = 0u;
        }
    }
}

struct BusParams {
    uint32_t var_bus, tuple_bus, bitwise_bus;
    uint32_t* var_hist;
    uint32_t* tuple_hist;
    uint32_t* bitwise_hist;
    uint32_t var_bins, tuple_sz0, tuple_sz1;
    const uint32_t* slot_range;  // binned mode: per item slot, the expected partitions (in_expected_partitions)
};

// Layout of BitwiseOperationLookup<8>'s count buffer (EXTERNAL to the reference
// checkout, assumption A3 of SURVEY.md): 2^16 range counters followed by 2^16 xor
// counters, both indexed by x * 256 + y.
__host__ __device__ __forceinline__ uint32_t bitwise_index(uint32_t x, uint32_t y, uint32_t selector) {
    return selector * (1u << (2 * POWDR_BITWISE_NUM_BITS)) + (x << POWDR_BITWISE_NUM_BITS) + y;
}

// Binned mode (long traces). The device-wide atomic rate (27 G/s on MI355X, any scope, see
// profiles/r01_microbench_atomics.txt) would bound this stage at ~1 atomic per lookup, and hot bins
// (bytes that are mostly 0, constant range widths) serialise far below that. Instead the
// evaluation kernel writes one packed item (bin | multiplicity << 20) per (periphery interaction,
// row) into a dense buffer — coalesced, no atomics — and a second kernel counts the items of
// one 32 K-bin partition of one table in an LDS histogram (LDS atomics), touching global
// memory with one atomicAdd per non-empty bin per workgroup.
constexpr uint32_t kItemNone = 0xffffffffu;
constexpr uint32_t kItemBinBits = 20;
constexpr uint32_t kItemMaxMult = 1u << (32 - kItemBinBits);
constexpr uint32_t kPartBins = 32768;  // bins per histogram partition: 128 KB of LDS counters

// The partitions of its table a slot's items are EXPECTED in, as (first | last << 16), decided at plan time from the
// constant operands of the interaction (a 12-14-bit range check belongs to partition 0, a bitwise lookup with a
// constant operation to two of four); the histogram pass of a partition skips the slots whose range excludes it. An
// item that falls outside its slot's range (only a dishonest trace produces one) is not packed but counted directly
// with a global atomic, so the result is exact either way.
__device__ __forceinline__ bool in_expected_partitions(uint32_t range, uint32_t bin) {
    const uint32_t part = bin / kPartBins;
    return part >= (range & 0xffffu) && part <= (range >> 16);
}

template <bool BINNED>
__global__ __launch_bounds__(kBlock) void apc_apply_bus_kernel(
    const uint32_t* __restrict__ trace, int num_calls, const uint32_t* __restrict__ bytecode,
    const DevInteraction* __restrict__ interactions, uint32_t n_interactions,
    const ExprSpan* __restrict__ spans, BusParams p, uint32_t per_chunk,
    const int32_t* __restrict__ slot_of, uint32_t* __restrict__ items, size_t item_stride, size_t col_stride,
    size_t row0) {
    __shared__ uint32_t stack_lds[pw::kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t rl = (size_t)blockIdx.x * kBlock + threadIdx.x;  // row within this launch's row window
    const size_t r = row0 + rl;
    const bool live = r < (size_t)num_calls;
    if (!BINNED && !live) return;
    if (BINNED && rl >= item_stride) return;
    const uint32_t i0 = blockIdx.y * per_chunk;
    const uint32_t i1 = min(n_interactions, i0 + per_chunk);

    for (uint32_t i = i0; i < i1; ++i) {
        const DevInteraction intr = interactions[i];
        int kind;
        if (intr.bus_id == p.var_bus) kind = 0;
        else if (intr.bus_id == p.tuple_bus) kind = 1;
        else if (intr.bus_id == p.bitwise_bus) kind = 2;
        else continue;  // execution bridge / memory / pc lookup: no periphery side effect

        const uint32_t range = BINNED ? p.slot_range[slot_of[i]] : 0u;
        uint32_t bin = kItemNone, m = 0u;
        uint32_t* table = kind == 0 ? p.var_hist : kind == 1 ? p.tuple_hist : p.bitwise_hist;
        if (live) {
            const ExprSpan* sp = spans + intr.args_index_off;
            const ExprSpan ms = sp[0];
            m = bb::from_monty(pw::eval_expr<kBlock, true>(bytecode + ms.off, ms.len, trace, r, stk, col_stride));
            if (m != 0u) {
                const ExprSpan s0 = sp[1], s1 = sp[2];
                const uint32_t a0 = bb::from_monty(pw::eval_expr<kBlock, true>(bytecode + s0.off, s0.len, trace, r, stk, col_stride));
                const uint32_t a1 = bb::from_monty(pw::eval_expr<kBlock, true>(bytecode + s1.off, s1.len, trace, r, stk, col_stride));
                if (kind == 0) {
                    // [value, max_bits] -> bin (1 << max_bits) + value - 1   (apc_apply_bus.cu:74)
                    // (shift counts >= 32 give 0, as PTX shl.b32 does for the reference build)
                    const uint32_t idx = (a1 < 32u ? (1u << a1) : 0u) + a0 - 1u;
                    if (idx < p.var_bins) bin = idx;
                } else if (kind == 1) {
                    // [v0, v1] -> bin v0 * sz1 + v1                         (apc_apply_bus.cu:89)
                    const uint32_t idx = a0 * p.tuple_sz1 + a1;
                    if (idx < p.tuple_sz0 * p.tuple_sz1) bin = idx;
                } else {
                    // [x, y, x_xor_y, selector]; arg 2 is never read (apc_apply_bus.cu:94-99)
                    const ExprSpan s3 = sp[4];
                    const uint32_t sel = bb::from_monty(pw::eval_expr<kBlock, true>(bytecode + s3.off, s3.len, trace, r, stk, col_stride));
                    if (sel <= 1u && a0 < 256u && a1 < 256u) bin = bitwise_index(a0, a1, sel);
                }
            }
        }
        if (BINNED) {
            uint32_t item = kItemNone;
            if (bin != kItemNone) {
                if (m < kItemMaxMult - 1u && bin < (1u << kItemBinBits) && in_expected_partitions(range, bin)) item = bin | (m << kItemBinBits);  // m = kItemMaxMult-1 could encode kItemNone: counted directly
                else atomicAdd(table + bin, m);  // does not fit the packed item: rare, direct
            }
            items[(size_t)slot_of[i] * item_stride + rl] = item;
        } else if (bin != kItemNone) {
            atomicAdd(table + bin, m);
        }
    }
}

// The same replay on plan-compiled xbc code (xbc.hpp): only periphery interactions are listed,
// with their table, item slot and the four expression spans resolved on the host.
struct XInteraction {
    uint32_t kind;    // 0 var-range, 1 tuple2, 2 bitwise
    uint32_t slot;    // item slot (binned mode)
    uint32_t off[4];  // instruction offsets of mult, arg0, arg1, selector
    uint32_t len[4];
};

template <bool BINNED>
__global__ __launch_bounds__(kBlock) void apc_apply_bus_xbc_kernel(
    const uint32_t* __restrict__ trace, int num_calls, const uint32_t* __restrict__ code,
    const XInteraction* __restrict__ xint, uint32_t n_xint, BusParams p, uint32_t per_chunk,
    uint32_t* __restrict__ items, size_t item_stride, size_t col_stride, size_t row0) {
    __shared__ uint32_t stack_lds[pw::kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const size_t rl = (size_t)blockIdx.x * kBlock + threadIdx.x;  // row within this launch's row window
    const size_t r = row0 + rl;
    const bool live = r < (size_t)num_calls;
    if (!BINNED && !live) return;
    if (BINNED && rl >= item_stride) return;
    const uint32_t i0 = blockIdx.y * per_chunk;
    const uint32_t i1 = min(n_xint, i0 + per_chunk);
    for (uint32_t i = i0; i < i1; ++i) {
        const XInteraction xi = xint[i];
        const uint32_t range = BINNED ? p.slot_range[xi.slot] : 0u;
        uint32_t bin = kItemNone, m = 0u;
        uint32_t* table = xi.kind == 0 ? p.var_hist : xi.kind == 1 ? p.tuple_hist : p.bitwise_hist;
        if (live) {
            m = bb::from_monty(xbc::eval<kBlock, true>(code + 2 * (size_t)xi.off[0], xi.len[0], trace, r, stk, col_stride));
            if (m != 0u) {
                const uint32_t a0 = bb::from_monty(xbc::eval<kBlock, true>(code + 2 * (size_t)xi.off[1], xi.len[1], trace, r, stk, col_stride));
                const uint32_t a1 = bb::from_monty(xbc::eval<kBlock, true>(code + 2 * (size_t)xi.off[2], xi.len[2], trace, r, stk, col_stride));
                if (xi.kind == 0) {
                    const uint32_t idx = (a1 < 32u ? (1u << a1) : 0u) + a0 - 1u;
                    if (idx < p.var_bins) bin = idx;
                } else if (xi.kind == 1) {
                    const uint32_t idx = a0 * p.tuple_sz1 + a1;
                    if (idx < p.tuple_sz0 * p.tuple_sz1) bin = idx;
                } else {
                    const uint32_t sel = bb::from_monty(xbc::eval<kBlock, true>(code + 2 * (size_t)xi.off[3], xi.len[3], trace, r, stk, col_stride));
                    if (sel <= 1u && a0 < 256u && a1 < 256u) bin = bitwise_index(a0, a1, sel);
                }
            }
        }
        if (BINNED) {
            uint32_t item = kItemNone;
            if (bin != kItemNone) {
                if (m < kItemMaxMult - 1u && bin < (1u << kItemBinBits) && in_expected_partitions(range, bin)) item = bin | (m << kItemBinBits);  // m = kItemMaxMult-1 could encode kItemNone: counted directly
                else atomicAdd(table + bin, m);
            }
            items[(size_t)xi.slot * item_stride + rl] = item;
        } else if (bin != kItemNone) {
            atomicAdd(table + bin, m);
        }
    }
}

// Interactions whose multiplicity and arguments are all small forms (small_form.hpp): no interpreter. All cells an
// interaction reads are requested before the first one is used, so an interaction costs one memory round trip instead
// of one per bytecode instruction.
struct FastInteraction {
    uint32_t kind;  // 0 var-range, 1 tuple2, 2 bitwise
    uint32_t slot;  // item slot (binned mode)
    uint32_t pad[2];
    pw::SmallForm f[4];  // mult, arg0, arg1, selector (bitwise only)
};

template <bool BINNED>
__global__ __launch_bounds__(kBlock) void apc_apply_bus_fast_kernel(
    const uint32_t* __restrict__ trace, int num_calls, const FastInteraction* __restrict__ fint, uint32_t n_fint, BusParams p,
    uint32_t per_chunk, uint32_t* __restrict__ items, size_t item_stride, size_t col_stride, size_t row0) {
    const size_t rl = (size_t)blockIdx.x * kBlock + threadIdx.x;  // row within this launch's row window
    const size_t r = row0 + rl;
    const bool live = r < (size_t)num_calls;
    if (!BINNED && !live) return;
    if (BINNED && rl >= item_stride) return;
    const size_t rr = live ? r : 0;  // dead rows read row 0 and discard it
    const uint32_t i0 = blockIdx.y * per_chunk;
    const uint32_t i1 = min(n_fint, i0 + per_chunk);
    for (uint32_t i = i0; i < i1; ++i) {
        const FastInteraction fi = fint[i];
        const uint32_t range = BINNED ? p.slot_range[fi.slot] : 0u;
        uint32_t ta[4], tb[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ta[k] = (fi.f[k].flags & pw::SmallForm::USES_A) ? trace[(size_t)fi.f[k].a * col_stride + rr] : 0u;
            tb[k] = (fi.f[k].flags & pw::SmallForm::USES_B) ? trace[(size_t)fi.f[k].b * col_stride + rr] : 0u;
        }
        uint32_t bin = kItemNone;
        const uint32_t m = live ? bb::from_monty(fi.f[0].eval(ta[0], tb[0])) : 0u;
        uint32_t* table = fi.kind == 0 ? p.var_hist : fi.kind == 1 ? p.tuple_hist : p.bitwise_hist;
        if (m != 0u) {
            const uint32_t a0 = bb::from_monty(fi.f[1].eval(ta[1], tb[1]));
            const uint32_t a1 = bb::from_monty(fi.f[2].eval(ta[2], tb[2]));
            if (fi.kind == 0) {
                const uint32_t idx = (a1 < 32u ? (1u << a1) : 0u) + a0 - 1u;
                if (idx < p.var_bins) bin = idx;
            } else if (fi.kind == 1) {
                const uint32_t idx = a0 * p.tuple_sz1 + a1;
                if (idx < p.tuple_sz0 * p.tuple_sz1) bin = idx;
            } else {
                const uint32_t sel = bb::from_monty(fi.f[3].eval(ta[3], tb[3]));
                if (sel <= 1u && a0 < 256u && a1 < 256u) bin = bitwise_index(a0, a1, sel);
            }
        }
        if (BINNED) {
            uint32_t item = kItemNone;
            if (bin != kItemNone) {
                if (m < kItemMaxMult - 1u && bin < (1u << kItemBinBits) && in_expected_partitions(range, bin)) item = bin | (m << kItemBinBits);  // m = kItemMaxMult-1 could encode kItemNone: counted directly
                else atomicAdd(table + bin, m);
            }
            items[(size_t)fi.slot * item_stride + rl] = item;
        } else if (bin != kItemNone) {
            atomicAdd(table + bin, m);
        }
    }
}

constexpr int kHistBlock = 1024;

__global__ __launch_bounds__(kHistBlock) void bus_histogram_kernel(
    const uint32_t* __restrict__ items, size_t item_stride, const uint32_t* __restrict__ slots, uint32_t n_slots,
    uint32_t* __restrict__ hist, uint32_t bins, uint32_t rows_per_chunk, const uint32_t* __restrict__ slot_range) {
    __shared__ uint32_t lh[kPartBins];
    const uint32_t bin0 = blockIdx.x * kPartBins;
    for (uint32_t b = threadIdx.x; b < kPartBins; b += kHistBlock) lh[b] = 0u;
    __syncthreads();
    const size_t r0 = (size_t)blockIdx.y * rows_per_chunk;
    const size_t r1 = r0 + rows_per_chunk < item_stride ? r0 + rows_per_chunk : item_stride;
    for (uint32_t s = 0; s < n_slots; ++s) {
        const uint32_t range = slot_range[slots[s]];
        if (blockIdx.x < (range & 0xffffu) || blockIdx.x > (range >> 16)) continue;  // no item of this slot lands here
        const uint4* it = reinterpret_cast<const uint4*>(items + (size_t)slots[s] * item_stride);
        for (size_t q = (r0 >> 2) + threadIdx.x; q < (r1 >> 2); q += kHistBlock) {
            const uint4 v = it[q];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            // lanes of this iteration (the last one of a chunk may be partial) and the first of them
            const unsigned long long active = __builtin_amdgcn_ballot_w64(true);
            const bool leader = (unsigned)__lane_id() == (unsigned)__builtin_ctzll(active);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t b = (w[k] & ((1u << kItemBinBits) - 1u)) - bin0;
                const bool hit = w[k] != kItemNone && b < kPartBins;
                // a slot fed from a cell that does not change from row to row sends ONE item 64 times: one LDS atomic for the wave
                // instead of 64 that conflict (same-address LDS atomics of one instruction are serialised)
                if (__builtin_amdgcn_ballot_w64(w[k] != (uint32_t)__builtin_amdgcn_readfirstlane((int)w[k])) == 0ull) {
                    if (hit && leader) atomicAdd(&lh[b], (w[k] >> kItemBinBits) * (uint32_t)__builtin_popcountll(active));
                } else if (hit) {
                    atomicAdd(&lh[b], w[k] >> kItemBinBits);
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kPartBins; b += kHistBlock) {
        const uint32_t c = lh[b];
        if (c && bin0 + b < bins) atomicAdd(hist + bin0 + b, c);
    }
}

// host-side classification of the interaction list, cached by content (plan_cache.hpp). Every table is an allocation of its own
// with spare entries at its end (+1 entry, +2 words on the xbc code): the kernels may read them.
struct BusPlan {
    pw::DeviceBuf slot_of;   // int32_t per interaction: item slot or -1
    pw::DeviceBuf slots[3];  // uint32_t slot ids per table (var, tuple, bitwise)
    uint32_t n_slots[3] = {0, 0, 0};
    uint32_t total_slots = 0;
    // xbc form of the periphery interactions (absent if some expression did not compile)
    bool has_xbc = false;
    pw::DeviceBuf xint, code;  // XInteraction, xbc words
    // the same interactions split into those that are small forms throughout (fast kernel) and the rest (interpreter)
    pw::DeviceBuf slot_range;  // uint32_t per item slot: expected partitions (first | last << 16)
    pw::DeviceBuf fint, xint_slow;  // FastInteraction, XInteraction
    uint32_t n_fast = 0, n_slow = 0;
};
// keyed by the three host tables, the three bus ids and the device
pw::PlanCache<BusPlan> g_bus_plans(64);

// item buffer of the binned path: one per host thread (= per launch stream)
struct ItemBuffer {
    uint32_t* p = nullptr;
    size_t words = 0;
    int device = -1;  // the device the buffer lives on (a host thread may move to another GPU)
    ~ItemBuffer() { if (p) (void)hipFree(p); }  // a host thread that exits gives its buffer back
    // false: the allocation failed (the caller falls through to the direct path)
    bool ensure(int on_device, size_t need) {
        if (need <= words && device == on_device) return true;
        device = on_device;
        if (p) (void)hipFree(p);
        p = nullptr; words = 0;
        if (hipMalloc(&p, need * 4) != hipSuccess) { (void)hipGetLastError(); return false; }
        words = need;
        return true;
    }
};
thread_local ItemBuffer g_item_buf;

// The replay's knobs, read from the environment on every call (unset = default).
struct BusKnobs {
    int binned = -1;   // POWDR_BUS_BINNED; unset: by the length of the trace
    bool xbc = true;   // POWDR_BUS_XBC=0: walk the reference's post-fix bytecode
    bool fast = true;  // POWDR_BUS_FAST=0: small-form interactions go through the interpreter too
    bool want_binned(int num_apc_calls) const { return binned < 0 ? num_apc_calls >= 16384 : binned != 0; }
    static BusKnobs from_env() {
        BusKnobs k;
        if (const char* e = getenv("POWDR_BUS_BINNED")) k.binned = atoi(e) != 0;
        if (const char* e = getenv("POWDR_BUS_XBC")) k.xbc = atoi(e) != 0;
        if (const char* e = getenv("POWDR_BUS_FAST")) k.fast = atoi(e) != 0;
        return k;
    }
};

// host views of the tables a plan is compiled from: the caller's own memory (powdr_apc_apply_bus_host_tables) or copies fetched
// from the device (reference entry)
struct BusTables {
    const DevInteraction* inter; size_t n_inter;
    const ExprSpan* spans; size_t n_spans;
    const uint32_t* bc; size_t bc_len;
    uint32_t ids[3];  // var-range, tuple2, bitwise bus
};

int build_bus_plan(const BusTables& t, const uint32_t table_bins[3], BusPlan& bp) {
    std::vector<int32_t> slot_of(t.n_inter, -1);
    std::vector<uint32_t> per_table[3];
    std::vector<XInteraction> xints, xints_slow;
    std::vector<uint32_t> slot_range;
    std::vector<FastInteraction> fints;
    std::vector<uint32_t> code;
    xbc::Compiler cc;
    bool ok = true;
    for (size_t i = 0; i < t.n_inter; ++i) {
        const DevInteraction& in = t.inter[i];
        int kind = in.bus_id == t.ids[0] ? 0 : in.bus_id == t.ids[1] ? 1 : in.bus_id == t.ids[2] ? 2 : -1;
        if (kind < 0) continue;
        slot_of[i] = (int32_t)bp.total_slots;
        XInteraction xi{};
        xi.kind = (uint32_t)kind;
        xi.slot = bp.total_slots;
        per_table[kind].push_back(bp.total_slots++);
        const uint32_t which[4] = {0, 1, 2, 4};  // mult, arg0, arg1, (bitwise) selector = arg 3
        FastInteraction fi{};
        fi.kind = (uint32_t)kind;
        fi.slot = xi.slot;
        fi.f[3].flags = pw::SmallForm::IS_CONST;
        bool fast = true;
        for (int k = 0; k < (kind == 2 ? 4 : 3) && ok; ++k) {
            const size_t si = (size_t)in.args_index_off + which[k];
            if (si >= t.n_spans || (size_t)t.spans[si].off + t.spans[si].len > t.bc_len) { ok = false; break; }
            xi.off[k] = (uint32_t)(code.size() / 2);
            if (!cc.compile(t.bc + t.spans[si].off, t.spans[si].len, code)) { ok = false; break; }
            xi.len[k] = (uint32_t)(code.size() / 2) - xi.off[k];
            fast = fast && pw::analyze_small_form(t.bc + t.spans[si].off, t.spans[si].len, fi.f[k]);
        }
        xints.push_back(xi);
        if (fast) fints.push_back(fi);
        else xints_slow.push_back(xi);
        // expected partitions of this slot's items
        uint32_t first = 0, last = (table_bins[kind] - 1) / kPartBins;
        if (ok) {
            pw::SmallForm c;
            const auto constant_arg = [&](uint32_t arg, uint32_t& value) {
                const size_t si = (size_t)in.args_index_off + arg;
                if (!pw::analyze_small_form(t.bc + t.spans[si].off, t.spans[si].len, c) || !(c.flags & pw::SmallForm::IS_CONST)) return false;
                value = bb::from_monty(c.k0);
                return true;
            };
            uint32_t v;
            if (kind == 0 && constant_arg(2, v) && v < 31) {  // honest values of a `v`-bit check: [2^v - 1, 2^(v+1) - 2]
                first = ((1u << v) - 1u) / kPartBins;
                last = std::min(last, ((2u << v) - 2u) / kPartBins);
                if (first > last) first = last;
            } else if (kind == 2 && constant_arg(4, v) && v <= 1) {
                first = bitwise_index(0, 0, v) / kPartBins;
                last = bitwise_index(255, 255, v) / kPartBins;
            }
        }
        slot_range.push_back(first | (last << 16));
    }
    if (int rc = pw::upload_table(bp.slot_range, slot_range.data(), slot_range.size(), 1)) return rc;
    if (int rc = pw::upload_table(bp.slot_of, slot_of.data(), slot_of.size(), 1)) return rc;
    for (int k = 0; k < 3; ++k) {
        bp.n_slots[k] = (uint32_t)per_table[k].size();
        if (int rc = pw::upload_table(bp.slots[k], per_table[k].data(), per_table[k].size(), 1)) return rc;
    }
    if (ok && !xints.empty()) {
        if (int rc = pw::upload_table(bp.xint, xints.data(), xints.size())) return rc;
        if (int rc = pw::upload_table(bp.code, code.data(), code.size(), 2)) return rc;
        bp.has_xbc = true;
        bp.n_fast = (uint32_t)fints.size();
        bp.n_slow = (uint32_t)xints_slow.size();
        if (int rc = pw::upload_table(bp.fint, fints.data(), fints.size(), 1)) return rc;
        if (int rc = pw::upload_table(bp.xint_slow, xints_slow.data(), xints_slow.size(), 1)) return rc;
    }
    return 0;
}

// chunking of an interaction list over blockIdx.y so that short traces still fill the chip
struct Chunking { unsigned chunks = 1; uint32_t per_chunk = 1; };
Chunking chunking(unsigned row_blocks, uint32_t n_list) {
    const unsigned want_blocks = 256u * 8u;  // enough workgroups to cover 256 CUs x 8 blocks even for short traces
    Chunking c;
    if (n_list == 0) return c;
    if (row_blocks < want_blocks) {
        c.chunks = (want_blocks + row_blocks - 1) / row_blocks;
        const unsigned max_chunks = (n_list + 15) / 16;
        if (c.chunks > max_chunks) c.chunks = max_chunks;
        if (c.chunks > 65535u) c.chunks = 65535u;
        if (c.chunks == 0) c.chunks = 1;
    }
    c.per_chunk = (n_list + c.chunks - 1) / c.chunks;
    c.chunks = (n_list + c.per_chunk - 1) / c.per_chunk;
    return c;
}

// What the walkers of one call run over. The interpreter walks all periphery interactions (xbc), only the non-small-form ones
// (fast mode), or the reference's full list (post-fix mode).
struct Walk {
    const uint32_t* trace; int num_calls; size_t col_stride;
    BusParams p;
    const uint32_t* d_bytecode; const DevInteraction* d_interactions; uint32_t n_interactions; const ExprSpan* d_arg_spans;  // post-fix mode
    bool use_xbc, use_fast;
    const XInteraction* x_list; uint32_t n_x;
    Chunking x, f;
};

// the fast kernel, then the xbc kernel or the post-fix kernel, over `row_blocks` blocks of rows from row0. BINNED: into `items`
template <bool BINNED>
void launch_walkers(const BusPlan& plan, const Walk& w, unsigned row_blocks, uint32_t* items, size_t stride, size_t row0) {
    pw::ScopedKernelTimer t("apc_apply_bus_kernel");
    if (w.use_fast && plan.n_fast)
        hipLaunchKernelGGL(apc_apply_bus_fast_kernel<BINNED>, dim3(row_blocks, w.f.chunks), dim3(kBlock), 0, pw::stream(), w.trace,
                           w.num_calls, plan.fint.as<FastInteraction>(), plan.n_fast, w.p, w.f.per_chunk, items, stride, w.col_stride, row0);
    if (w.use_xbc) {
        if (w.n_x)
            hipLaunchKernelGGL(apc_apply_bus_xbc_kernel<BINNED>, dim3(row_blocks, w.x.chunks), dim3(kBlock), 0, pw::stream(), w.trace,
                               w.num_calls, plan.code.as<uint32_t>(), w.x_list, w.n_x, w.p, w.x.per_chunk, items, stride, w.col_stride, row0);
    } else
        hipLaunchKernelGGL(apc_apply_bus_kernel<BINNED>, dim3(row_blocks, w.x.chunks), dim3(kBlock), 0, pw::stream(), w.trace,
                           w.num_calls, w.d_bytecode, w.d_interactions, w.n_interactions, w.d_arg_spans, w.p, w.x.per_chunk,
                           BINNED ? plan.slot_of.as<int32_t>() : nullptr, items, stride, w.col_stride, row0);
}

// one 128-KB-LDS workgroup fits per CU, and the three launches run one after the other, so each launch gets ~2 x 256 workgroups
// of its own: partitions x row chunks
void launch_histograms(const BusPlan& plan, const uint32_t* items, size_t stride, uint32_t* const tables[3], const uint32_t table_bins[3]) {
    for (int t = 0; t < 3; ++t) {
        if (!plan.n_slots[t]) continue;
        const unsigned parts = pw::div_up(table_bins[t], kPartBins);
        unsigned n_chunks = (512 + parts - 1) / parts;
        const unsigned max_chunks = pw::div_up(stride, 4096);
        if (n_chunks > max_chunks) n_chunks = max_chunks;
        if (n_chunks == 0) n_chunks = 1;
        const uint32_t rows_per_chunk = (uint32_t)(((stride + n_chunks - 1) / n_chunks + 3) & ~(size_t)3);
        n_chunks = pw::div_up(stride, rows_per_chunk);
        pw::ScopedKernelTimer tt("bus_histogram_kernel");
        hipLaunchKernelGGL(bus_histogram_kernel, dim3(parts, n_chunks), dim3(kHistBlock), 0, pw::stream(), items, stride,
                           plan.slots[t].as<uint32_t>(), plan.n_slots[t], tables[t], table_bins[t], rows_per_chunk,
                           plan.slot_range.as<uint32_t>());
    }
}

}  // namespace

namespace {
int apply_derived_impl(PowdrFp* d_output, size_t H, int num_apc_calls, const DerivedExprSpec* d_specs, size_t n_cols,
                       const uint32_t* d_bytecode, size_t col_stride) {
    if (n_cols == 0) return 0;  // apc_tracegen.cu:114
    (void)hipGetLastError();    // do not report a stale error of an unrelated earlier call
    if (H == 0) return (int)hipGetLastError();
    unsigned g = pw::div_up(H, kBlock);
    if (g > 65535u * 16u) g = 65535u * 16u;
    pw::ScopedKernelTimer t("apc_apply_derived_expr_kernel");
    hipLaunchKernelGGL(apc_apply_derived_expr_kernel, dim3(g), dim3(kBlock), 0, pw::stream(),
                       d_output, H, num_apc_calls, d_specs, n_cols, d_bytecode, col_stride);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int _apc_apply_derived_expr(PowdrFp* d_output, size_t H, int num_apc_calls,
                                       const DerivedExprSpec* d_specs, size_t n_cols,
                                       const uint32_t* d_bytecode) {
    return apply_derived_impl(d_output, H, num_apc_calls, d_specs, n_cols, d_bytecode, 1);
}

extern "C" int powdr_apc_apply_derived_expr_cols(PowdrFp* d_output, size_t H, int num_apc_calls,
                                                 const DerivedExprSpec* d_specs, size_t n_cols,
                                                 const uint32_t* d_bytecode) {
    return apply_derived_impl(d_output, H, num_apc_calls, d_specs, n_cols, d_bytecode, H);
}

namespace {
int apply_bus_impl(const PowdrFp* d_output, int num_apc_calls,
                   const uint32_t* d_bytecode, size_t bytecode_len,
                   const DevInteraction* d_interactions, size_t n_interactions,
                   const ExprSpan* d_arg_spans, size_t n_arg_spans,
                   uint32_t var_range_bus_id, uint32_t* d_var_hist, size_t var_num_bins,
                   uint32_t tuple2_bus_id, uint32_t* d_tuple2_hist, uint32_t tuple2_sz0,
                   uint32_t tuple2_sz1, uint32_t bitwise_bus_id,
                   uint32_t* d_bitwise_hist, size_t col_stride, const uint32_t* h_bytecode = nullptr,
                   const DevInteraction* h_interactions = nullptr, const ExprSpan* h_arg_spans = nullptr) {
    if (num_apc_calls <= 0) return 0;  // apc_apply_bus.cu:146
    (void)hipGetLastError();
    if (n_interactions == 0) return (int)hipGetLastError();
    const BusKnobs knobs = BusKnobs::from_env();
    const uint32_t table_bins[3] = {(uint32_t)var_num_bins, tuple2_sz0 * tuple2_sz1, 2u << (2 * POWDR_BITWISE_NUM_BITS)};
    uint32_t* const tables[3] = {d_var_hist, d_tuple2_hist, d_bitwise_hist};

    // ---- tables: the caller's on the host (powdr_apc_apply_bus_host_tables: no copy, no synchronisation), or fetched ----
    BusTables t{h_interactions, n_interactions, h_arg_spans, n_arg_spans, h_bytecode, bytecode_len,
                {var_range_bus_id, tuple2_bus_id, bitwise_bus_id}};
    std::vector<DevInteraction> h;
    std::vector<ExprSpan> hs;
    std::vector<uint32_t> hb;
    if (!(h_bytecode && h_interactions && (h_arg_spans || !n_arg_spans))) {
        h.resize(n_interactions); hs.resize(n_arg_spans); hb.resize(bytecode_len);
        PW_HIP_TRY(hipMemcpyAsync(h.data(), d_interactions, n_interactions * sizeof(DevInteraction), hipMemcpyDeviceToHost, pw::stream()));
        if (n_arg_spans) PW_HIP_TRY(hipMemcpyAsync(hs.data(), d_arg_spans, n_arg_spans * sizeof(ExprSpan), hipMemcpyDeviceToHost, pw::stream()));
        if (bytecode_len) PW_HIP_TRY(hipMemcpyAsync(hb.data(), d_bytecode, bytecode_len * 4, hipMemcpyDeviceToHost, pw::stream()));
        PW_HIP_TRY(hipStreamSynchronize(pw::stream()));
        t.inter = h.data(); t.spans = hs.data(); t.bc = hb.data();
    }

    // ---- plan ----
    int device = 0;
    PW_HIP_TRY(hipGetDevice(&device));
    std::shared_ptr<const BusPlan> plan;
    if (int rc = g_bus_plans.get({pw::key_part(t.inter, t.n_inter), pw::key_part(t.spans, t.n_spans), pw::key_part(t.bc, t.bc_len),
                                  pw::key_value(t.ids), pw::key_value(device)},
                                 [&](BusPlan& bp) { return build_bus_plan(t, table_bins, bp); }, plan))
        return rc;
    if (plan->total_slots == 0) return (int)hipGetLastError();

    Walk w;
    w.trace = d_output; w.num_calls = num_apc_calls; w.col_stride = col_stride;
    w.p.var_bus = var_range_bus_id; w.p.tuple_bus = tuple2_bus_id; w.p.bitwise_bus = bitwise_bus_id;
    w.p.var_hist = d_var_hist; w.p.tuple_hist = d_tuple2_hist; w.p.bitwise_hist = d_bitwise_hist;
    w.p.var_bins = (uint32_t)var_num_bins; w.p.tuple_sz0 = tuple2_sz0; w.p.tuple_sz1 = tuple2_sz1;
    w.p.slot_range = nullptr;
    w.d_bytecode = d_bytecode; w.d_interactions = d_interactions; w.n_interactions = (uint32_t)n_interactions; w.d_arg_spans = d_arg_spans;
    w.use_xbc = knobs.xbc && plan->has_xbc;
    w.use_fast = w.use_xbc && knobs.fast;
    w.x_list = (w.use_fast ? plan->xint_slow : plan->xint).as<XInteraction>();
    w.n_x = w.use_fast ? plan->n_slow : plan->total_slots;
    const unsigned row_blocks = pw::div_up((size_t)num_apc_calls, kBlock);
    w.x = chunking(row_blocks, w.use_xbc ? w.n_x : (uint32_t)n_interactions);
    if (w.use_fast) w.f = chunking(row_blocks, plan->n_fast);

    // ---- stats ----
    uint64_t* stats = pw::call_stats();
    stats[pw::kStatBusFastInteractions] += w.use_fast ? plan->n_fast : 0;
    stats[pw::kStatBusInterpretedInteractions] += w.use_xbc ? w.n_x : plan->total_slots;
    stats[pw::kStatBusXbcCalls] += w.use_xbc ? 1 : 0;

    // ---- long traces: binned path ----
    if (knobs.want_binned(num_apc_calls) && table_bins[0] <= (1u << kItemBinBits) && table_bins[1] <= (1u << kItemBinBits)) {
        // rows are processed in windows of at most 2^20 so that the item buffer stays bounded
        // (slots x 4 MiB): a 2^22-row trace with 1 600 periphery interactions would otherwise need 27 GB
        const size_t all_rows = ((size_t)num_apc_calls + 3) & ~(size_t)3;
        const size_t window = all_rows < ((size_t)1 << 20) ? all_rows : ((size_t)1 << 20);
        if (g_item_buf.ensure(device, (size_t)plan->total_slots * window)) {
            w.p.slot_range = plan->slot_range.as<uint32_t>();
            for (size_t row0 = 0; row0 < all_rows; row0 += window) {
                const size_t stride = all_rows - row0 < window ? all_rows - row0 : window;
                stats[pw::kStatBusBinnedWindows] += 1;
                launch_walkers<true>(*plan, w, pw::div_up(stride, kBlock), g_item_buf.p, stride, row0);
                launch_histograms(*plan, g_item_buf.p, stride, tables, table_bins);
            }
            return (int)hipGetLastError();
        }
    }
    stats[pw::kStatBusDirectCalls] += 1;
    launch_walkers<false>(*plan, w, row_blocks, nullptr, 0, 0);
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int _apc_apply_bus(const PowdrFp* d_output, int num_apc_calls,
                              const uint32_t* d_bytecode, size_t bytecode_len,
                              const DevInteraction* d_interactions, size_t n_interactions,
                              const ExprSpan* d_arg_spans, size_t n_arg_spans,
                              uint32_t var_range_bus_id, uint32_t* d_var_hist, size_t var_num_bins,
                              uint32_t tuple2_bus_id, uint32_t* d_tuple2_hist, uint32_t tuple2_sz0,
                              uint32_t tuple2_sz1, uint32_t bitwise_bus_id,
                              uint32_t* d_bitwise_hist) {
    return apply_bus_impl(d_output, num_apc_calls, d_bytecode, bytecode_len, d_interactions, n_interactions, d_arg_spans,
                          n_arg_spans, var_range_bus_id, d_var_hist, var_num_bins, tuple2_bus_id, d_tuple2_hist, tuple2_sz0,
                          tuple2_sz1, bitwise_bus_id, d_bitwise_hist, 1);
}

extern "C" int powdr_apc_apply_bus_cols(const PowdrFp* d_output, size_t output_height, int num_apc_calls,
                                        const uint32_t* d_bytecode, size_t bytecode_len,
                                        const DevInteraction* d_interactions, size_t n_interactions,
                                        const ExprSpan* d_arg_spans, size_t n_arg_spans,
                                        uint32_t var_range_bus_id, uint32_t* d_var_hist, size_t var_num_bins,
                                        uint32_t tuple2_bus_id, uint32_t* d_tuple2_hist, uint32_t tuple2_sz0,
                                        uint32_t tuple2_sz1, uint32_t bitwise_bus_id,
                                        uint32_t* d_bitwise_hist) {
    return apply_bus_impl(d_output, num_apc_calls, d_bytecode, bytecode_len, d_interactions, n_interactions, d_arg_spans,
                          n_arg_spans, var_range_bus_id, d_var_hist, var_num_bins, tuple2_bus_id, d_tuple2_hist, tuple2_sz0,
                          tuple2_sz1, bitwise_bus_id, d_bitwise_hist, output_height);
}

// Extension: _apc_apply_bus for a caller that still holds the three tables on the host (powdr_apc_generate_witness_gpu
// compiles them itself): h_* are host copies of the device tables. Skips the device-to-host copy of the bytecode
// (megabytes for an un-optimised APC), its hash over the copy and the stream synchronisation of the reference entry.
// output_height = 0: PUSH_APC operands are element offsets (reference encoding); otherwise column indices.
extern "C" int powdr_apc_apply_bus_host_tables(const PowdrFp* d_output, size_t output_height, int num_apc_calls,
                                               const uint32_t* d_bytecode, const uint32_t* h_bytecode, size_t bytecode_len,
                                               const DevInteraction* d_interactions, const DevInteraction* h_interactions,
                                               size_t n_interactions, const ExprSpan* d_arg_spans, const ExprSpan* h_arg_spans,
                                               size_t n_arg_spans, uint32_t var_range_bus_id, uint32_t* d_var_hist,
                                               size_t var_num_bins, uint32_t tuple2_bus_id, uint32_t* d_tuple2_hist,
                                               uint32_t tuple2_sz0, uint32_t tuple2_sz1, uint32_t bitwise_bus_id,
                                               uint32_t* d_bitwise_hist) {
    if (!h_bytecode || !h_interactions || (n_arg_spans && !h_arg_spans)) return (int)hipErrorInvalidValue;
    return apply_bus_impl(d_output, num_apc_calls, d_bytecode, bytecode_len, d_interactions, n_interactions, d_arg_spans,
                          n_arg_spans, var_range_bus_id, d_var_hist, var_num_bins, tuple2_bus_id, d_tuple2_hist, tuple2_sz0,
                          tuple2_sz1, bitwise_bus_id, d_bitwise_hist, output_height ? output_height : 1, h_bytecode,
                          h_interactions, h_arg_spans);
}
