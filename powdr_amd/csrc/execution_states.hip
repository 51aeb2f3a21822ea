// The states of an execution from the instruction AIRs' traces (include/powdr_prover.h pw_execution_states_from_traces, DESIGN.md
// §5s): the pcs, the requested registers and the time keys of a segment's N + 1 states, kept on the device in the layout
// pw_apc_calls_from_states reads. The stages are register_states.hpp's; this file is the handle and the C entry points.
#include "register_states.hpp"

#include <memory>

namespace pw {

namespace {

namespace rs = register_states;

thread_local rs::Ctx g_es;  // (the arrays of the handle under construction are its `extra`)

}  // namespace

}  // namespace pw

using namespace pw;
using namespace pw::bus;

struct PwExecutionStates {
    DeviceBuf pcs, regs, keys;
    uint64_t n_states = 0, n_regs = 0, sends = 0;
    size_t bytes() const { return pcs.bytes + regs.bytes + keys.bytes; }
};

extern "C" void pw_execution_states_destroy(PwExecutionStates* e) { delete e; }

extern "C" void pw_execution_states_sizes(const PwExecutionStates* e, uint64_t* sizes) {
    if (!e || !sizes) return;
    sizes[0] = e->n_states;
    sizes[1] = e->n_regs;
    sizes[2] = e->sends;
    sizes[3] = e->bytes();
}

extern "C" void pw_execution_states_device(const PwExecutionStates* e, const uint32_t** d_pcs, const uint32_t** d_regs, const uint64_t** d_time_keys) {
    if (!e) return;
    if (d_pcs) *d_pcs = (const uint32_t*)e->pcs.p;
    if (d_regs) *d_regs = (const uint32_t*)e->regs.p;
    if (d_time_keys) *d_time_keys = (const uint64_t*)e->keys.p;
}

extern "C" int pw_execution_states_read(const PwExecutionStates* e, uint32_t* pcs, uint32_t* regs, uint64_t* time_keys) {
    if (!e) return -1;
    hipStream_t st = stream();
    if (pcs) PW_HIP_TRY(hipMemcpyAsync(pcs, e->pcs.p, e->n_states * 4, hipMemcpyDeviceToHost, st));
    if (regs && e->n_regs) PW_HIP_TRY(hipMemcpyAsync(regs, e->regs.p, e->n_regs * e->n_states * 4, hipMemcpyDeviceToHost, st));
    if (time_keys && e->n_states > 1) PW_HIP_TRY(hipMemcpyAsync(time_keys, e->keys.p, (e->n_states - 1) * 8, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

extern "C" void pw_execution_states_last_stats(uint64_t* out) {
    if (!out) return;
    out[0] = g_es.sends;
    out[1] = g_es.kept;
    out[2] = rs::kTile;
    out[3] = g_es.peak();
    out[4] = g_es.held();
}

extern "C" int pw_execution_states_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus, uint32_t memory_bus,
                                               uint32_t final_pc, uint32_t reg_as, uint32_t reg_ptr_step, const uint32_t* regs, size_t n_regs,
                                               const uint32_t* initial_regs, size_t scratch_bytes, PwExecutionStates** out, uint32_t* status, uint64_t* info) {
    const rs::Args a{airs, segment_of_air, n_airs, bridge_bus, memory_bus, final_pc, reg_as, reg_ptr_step};
    time_index::Bridge B;
    u64 slots = 0;
    if (!out || !status || !info || !rs::registers_ok(regs, n_regs, reg_ptr_step ? reg_ptr_step : 1u) || !rs::args_ok(a, &B, &slots)) return -1;
    rs::Ctx& cx = g_es;
    const ScratchCall call(cx, out, status, info);
    const size_t bound = call.bound(scratch_bytes);
    const size_t need = rs::bytes_needed(B.M, slots, n_regs);
    if (bound < need) {
        *status = 2;
        *info = need;  // (what is known before a row is read: every row may be active, every interaction a send)
        return 0;
    }
    auto result = std::make_unique<PwExecutionStates>();
    u64 N = 0;
    const int rc = rs::states_from_traces(a, std::vector<uint32_t>(regs, regs + n_regs), initial_regs, B, slots, cx, result->pcs, result->regs, result->keys, &N, status,
                                          info);
    if (rc || *status) return rc;
    result->n_states = N + 1;
    result->n_regs = n_regs;
    result->sends = cx.sends;
    *out = result.release();
    return 0;
}
