// The kernel that re-evaluates the tuples a list of packed witnesses names: for the two files that report tuples (bus_check.hip,
// system_traces.hip). A header of its own so that a file that only walks (empirical.hip) does not carry the kernel.
#pragma once
#include "bus_shared.hpp"

namespace pw {
namespace bus {

// args[e * stride + j] = argument j (canonical) of the interaction and row that witness e names, and with `mult` mult[e] = its
// multiplicity; witness e is wit[e * wit_stride] (a list of records that begin with their witness: the record's size in words). One
// wave per entry, every lane of it evaluating the same program on the same row (the interpreter wants wave-uniform code; the lists
// are short).
static __global__ __launch_bounds__(kBlock) void witness_args_kernel(const u64* __restrict__ wit, uint32_t wit_stride, u64 n, const AirDev* __restrict__ airs,
                                                                      uint32_t stride, uint32_t* __restrict__ args, uint32_t* __restrict__ mult) {
    __shared__ uint32_t stack_lds[kStackCap * kBlock];
    uint32_t* stk = stack_lds + threadIdx.x;
    const u64 e = (u64)blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (e >= n) return;
    const Witness w = unpack_witness(wit[e * wit_stride]);
    const AirDev a = airs[w.air];
    const LogupInteraction it = a.lp.d_inter[w.inter];
    const bool writer = (threadIdx.x & 63) == 0;
    if (mult) {
        const uint32_t v = eval_span_of(a, it.first_span, w.row, stk);
        if (writer) mult[e] = bb::from_monty(v);
    }
    for (uint32_t j = 0; j < it.n_args && j < stride; ++j) {
        const uint32_t v = eval_span_of(a, it.first_span + 1 + j, w.row, stk);
        if (writer) args[e * stride + j] = bb::from_monty(v);
    }
}

}  // namespace bus
}  // namespace pw
