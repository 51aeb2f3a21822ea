// How a kernel evaluates ONE multiplicity / argument of a bus interaction on one row — shared by the LogUp kernels of the prover
// (logup_kernels.hip) and the bus mock prover (bus_check.hip), so that both read an interaction exactly the same way.
#pragma once
#include "prover_internal.hpp"
#include "xbc.hpp"
#include "expr_eval.hpp"
#include "jit_device.hpp"

namespace pw {

constexpr int kLogupBlock = 256;  // lanes per workgroup of every kernel that calls eval_span (the stride of the interpreter's LDS stack)

// One multiplicity / argument on row r. FAST: the span's small form (k0 + k1 A + k2 B + k3 A B, fixed code, both loads issued at
// once, ~10 scalar instructions); else the xbc interpreter (a scalar decode of ~15 instructions per xbc instruction on the
// CU's one scalar unit, which is what bounds these kernels when it runs: PMC profiles/r02_pmc_logup_kernels.txt).
template <bool FAST>
__device__ __forceinline__ uint32_t eval_span(const LogupProgram& lp, uint32_t span, const uint32_t* __restrict__ m, size_t stride,
                                              size_t r, uint32_t* stk) {
    if (FAST && !(lp.d_forms[span].flags & SmallForm::NOT_SMALL)) {
        const SmallForm f = lp.d_forms[span];
        const uint32_t ta = (f.flags & SmallForm::USES_A) ? m[(size_t)f.a * stride + r] : 0u;
        const uint32_t tb = (f.flags & SmallForm::USES_B) ? m[(size_t)f.b * stride + r] : 0u;
        return f.eval(ta, tb);
    }
    const uint32_t off = lp.d_xspans[2 * span], len = lp.d_xspans[2 * span + 1];
    return xbc::eval<kLogupBlock, true>(lp.d_code + 2 * (size_t)off, len, m, r, stk, stride);
}

}  // namespace pw
