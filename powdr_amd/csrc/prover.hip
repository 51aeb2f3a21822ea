// pw-stark v0 prover: host orchestration of the HIP stages, Fiat-Shamir transcript, proof
// assembly. Protocol definition: oracle/stark_oracle.cpp (header comment) and DESIGN.md;
// the byte string produced here must equal the oracle's for the same trace.
//
// Data stays in HBM from the caller's trace to the last FRI layer; the host only sees
// 32-byte roots, the W+8 opened values and the query answers (a few hundred KB), which is
// what it needs to run the transcript.
#include "prover_state.hpp"
#include "prover_stages.hpp"
#include "xbc_compile.hpp"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <initializer_list>
#include <vector>

namespace pw {

namespace {

__global__ void gather_records_kernel(const uint32_t* __restrict__ arena, const uint64_t* __restrict__ offsets,
                                      uint32_t words_per_record, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * words_per_record) return;
    const uint32_t r = i / words_per_record, w = i - r * words_per_record;
    out[i] = arena[offsets[r] + w];
}

}  // namespace

int gather_records(const uint32_t* arena, const uint64_t* d_offsets, uint32_t words_per_record, uint32_t n, uint32_t* out) {
    if (!n) return 0;
    hipLaunchKernelGGL(gather_records_kernel, dim3(div_up((size_t)n * words_per_record, 256)), dim3(256), 0, stream(), arena, d_offsets,
                       words_per_record, n, out);
    return (int)hipGetLastError();
}

}  // namespace pw

using namespace pw;

extern "C" void pw_prover_destroy(PwProver* p);
extern "C" size_t pw_prover_device_bytes(const PwProver* p);
extern "C" int pw_prover_specialise(PwProver* p);
extern "C" int pw_prover_specialised(const PwProver* p, size_t* n_kernels, size_t* code_bytes, size_t* n_chunks);

// The row layout: the constraint programs of a row-aware AIR rewritten onto the compact device layout (prover_state.hpp
// PwProver::row_flags), one program after the other; fills next_cols, *row_cols and new spans. Operands are in bounds (checked before).
// Public values (operands 2 W1 + 3 + k) follow the compact columns: value k becomes operand W1 + *row_cols + k, so the
// device programs tell them from every column by one bound (PwProver::pub_base) whether or not the AIR is row-aware.
static std::vector<uint32_t> remap_row_programs(const uint32_t* bc, const uint32_t* spans, size_t n_constraints, uint32_t w1, uint32_t flags,
                                                std::vector<uint32_t>& next_cols, uint32_t* row_cols, std::vector<uint32_t>& new_spans) {
    // the next-row columns read, ascending (a sorted list, not a table of W1 entries: W1 comes from the caller)
    next_cols.clear();
    for (size_t k = 0; k < n_constraints; ++k)
        for (uint32_t ip = spans[2 * k], end = spans[2 * k] + spans[2 * k + 1]; ip < end;) {
            const uint32_t op = bc[ip++];
            if (op != POWDR_OP_PUSH_APC && op != POWDR_OP_PUSH_CONST) continue;
            const uint32_t a = bc[ip++];
            if (op == POWDR_OP_PUSH_APC && a >= w1 && a < 2 * w1) next_cols.push_back(a - w1);
        }
    std::sort(next_cols.begin(), next_cols.end());
    next_cols.erase(std::unique(next_cols.begin(), next_cols.end()), next_cols.end());
    auto slot = [&](uint32_t c) { return (uint32_t)(std::lower_bound(next_cols.begin(), next_cols.end(), c) - next_cols.begin()); };
    const uint32_t n_next = (uint32_t)next_cols.size();
    *row_cols = n_next + ((flags & pw::kRowsSelector) ? 3u : 0u);
    std::vector<uint32_t> out;
    new_spans.clear();
    for (size_t k = 0; k < n_constraints; ++k) {
        new_spans.push_back((uint32_t)out.size());
        new_spans.push_back(spans[2 * k + 1]);
        for (uint32_t ip = spans[2 * k], end = spans[2 * k] + spans[2 * k + 1]; ip < end;) {
            const uint32_t op = bc[ip++];
            out.push_back(op);
            if (op != POWDR_OP_PUSH_APC && op != POWDR_OP_PUSH_CONST) continue;
            uint32_t a = bc[ip++];
            if (op == POWDR_OP_PUSH_APC && a >= 2 * w1 + 3) a = w1 + *row_cols + (a - (2 * w1 + 3));
            else if (op == POWDR_OP_PUSH_APC && a >= w1) a = a < 2 * w1 ? w1 + slot(a - w1) : w1 + n_next + (a - 2 * w1);
            out.push_back(a);
        }
    }
    return out;
}

// `device` = false: host tables only (pw_jit_compile_check: code generation + hiprtc need no GPU). rows_w1 != 0: the row layout over
// rows_w1 (= width) columns — constraint operands below 2 rows_w1 + 3, is_transition of degree 0 — and behind them
// n_public public values of degree 0 (only with rows_w1)
static PwProver* create_prover(const PwStarkConfig* cfg, uint32_t width, const uint32_t* bc, size_t bc_len,
                               const uint32_t* spans, size_t n_constraints, bool device, uint32_t rows_w1 = 0, uint32_t n_public = 0) {
    if (!cfg || !width || (n_public && !rows_w1)) return nullptr;
    PwProver* p = new PwProver();
    p->cfg = *cfg;
    p->width = width;
    p->n_constraints = (uint32_t)n_constraints;
    p->h_spans.assign(spans, spans + 2 * n_constraints);
    const uint32_t bound = rows_w1 ? 2 * rows_w1 + 3 + n_public : width, deg0 = rows_w1 ? 2 * rows_w1 + 2 : 0xffffffffu;
    const uint32_t deg0_from = n_public ? 2 * rows_w1 + 3 : 0xffffffffu;
    p->n_public = n_public;
    for (size_t k = 0; k < n_constraints; ++k) {
        const uint32_t off = spans[2 * k], len = spans[2 * k + 1];
        const int d = (size_t)off + len <= bc_len ? pw::postfix_degree(bc + off, len, deg0, deg0_from) : pw::kBadDegree;
        // a span past the bytecode, an unknown opcode, an unbalanced or too deep stack, a column the trace does not have: no prover — the
        // post-fix fallback below is for well-formed programs the xbc compiler declines, not for these (they would index past the
        // bytecode or the trace on the device)
        if (d == pw::kBadDegree || !pw::postfix_columns_below(bc + off, len, bound)) { delete p; return nullptr; }
        if (d > p->max_degree) p->max_degree = d;
        if (rows_w1) p->row_flags |= pw::postfix_row_flags(bc + off, len, rows_w1);
    }
    // a row-aware AIR's programs go to the device (and to the xbc compiler) rewritten onto the compact layout of its values
    std::vector<uint32_t> row_bc, row_spans;
    if (p->row_flags || n_public) {
        row_bc = remap_row_programs(bc, spans, n_constraints, rows_w1, p->row_flags, p->h_next_cols, &p->row_cols, row_spans);
        bc = row_bc.data();
        bc_len = row_bc.size();
        spans = row_spans.data();
        if (n_public) p->pub_base = rows_w1 + p->row_cols;
    }
    // compile the post-fix constraint programs to xbc (xbc.hpp); fall back to the post-fix interpreter if
    // any program is malformed or too deep
    std::vector<uint32_t> code, xspans;
    bool ok = getenv("POWDR_QUOTIENT_XBC") ? atoi(getenv("POWDR_QUOTIENT_XBC")) != 0 : true;
    {
        xbc::Compiler cc;
        cc.pub_base = p->pub_base;
        for (size_t k = 0; k < n_constraints && ok; ++k) {
            const uint32_t off = spans[2 * k], len = spans[2 * k + 1];
            if ((size_t)off + len > bc_len) { ok = false; break; }
            const uint32_t o = (uint32_t)(code.size() / 2);
            if (!cc.compile(bc + off, len, code)) { ok = false; break; }
            xspans.push_back(o);
            xspans.push_back((uint32_t)(code.size() / 2) - o);
        }
    }
    const uint32_t* up_bc = ok ? code.data() : bc;
    const uint32_t* up_sp = ok ? xspans.data() : spans;
    const size_t up_bc_len = ok ? code.size() : bc_len;
    p->is_xbc = ok;
    if (ok) { p->h_xcode = code; p->h_xspans = xspans; }
    if (!device) return p;
    size_t bl = up_bc_len ? up_bc_len : 1, sl = n_constraints ? 2 * n_constraints : 1;
    if (hipMalloc(&p->d_bytecode, (bl + 2) * 4) != hipSuccess || hipMalloc(&p->d_spans, sl * 4) != hipSuccess) {
        delete p;
        return nullptr;
    }
    if (up_bc_len) (void)hipMemcpy(p->d_bytecode, up_bc, up_bc_len * 4, hipMemcpyHostToDevice);
    if (n_constraints) (void)hipMemcpy(p->d_spans, up_sp, 2 * n_constraints * 4, hipMemcpyHostToDevice);
    if (!p->h_next_cols.empty() && (hipMalloc(&p->d_next_cols, p->h_next_cols.size() * 4) != hipSuccess ||
                                    hipMemcpy(p->d_next_cols, p->h_next_cols.data(), p->h_next_cols.size() * 4, hipMemcpyHostToDevice) != hipSuccess)) {
        pw_prover_destroy(p);
        return nullptr;
    }
    if (n_public && hipMalloc(&p->d_pub, (size_t)n_public * 4) != hipSuccess) {
        pw_prover_destroy(p);
        return nullptr;
    }
    return p;
}

extern "C" PwProver* pw_prover_create(const PwStarkConfig* cfg, uint32_t width, const uint32_t* bc, size_t bc_len,
                                      const uint32_t* spans, size_t n_constraints) {
    return create_prover(cfg, width, bc, bc_len, spans, n_constraints, true);
}

// (interaction operands stay below `width` with the row layout too)
static PwProver* create_prover_logup(const PwStarkConfig* cfg, uint32_t width, const uint32_t* bc, size_t bc_len,
                                     const uint32_t* spans, size_t n_constraints, const uint32_t* inter, size_t n_inter,
                                     const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc, size_t ibc_len, bool device,
                                     uint32_t rows_w1 = 0, uint32_t n_public = 0) {
    PwProver* p = create_prover(cfg, width, bc, bc_len, spans, n_constraints, device, rows_w1, n_public);
    if (!p) return nullptr;
    // interactions: {bus, n_args, first span}; spans [mult, arg0, ...] into ibc (post-fix, column operands)
    std::vector<pw::LogupInteraction> li(n_inter);
    std::vector<uint32_t> xspans, code;
    std::vector<pw::SmallForm> forms;  // one per span; the few that are no small forms (sums of many flags, ...) stay with the interpreter
    size_t not_small = 0;
    xbc::Compiler cc;
    bool ok = pw::interaction_table_ok(inter, n_inter, ispans, n_ispans, ibc_len);
    for (size_t i = 0; i < n_inter && ok; ++i) {
        const uint32_t bus = inter[3 * i], na = inter[3 * i + 1], first = inter[3 * i + 2];
        li[i] = {bb::to_monty(bus % bb::P), na, (uint32_t)(xspans.size() / 2)};
        if (na > p->max_args) p->max_args = na;
        for (uint32_t k = 0; k <= na && ok; ++k) {
            const uint32_t off = ispans[2 * (first + k)], len = ispans[2 * (first + k) + 1];
            if (pw::postfix_degree(ibc + off, len) == pw::kBadDegree || !pw::postfix_columns_below(ibc + off, len, width)) { ok = false; break; }
            const uint32_t o = (uint32_t)(code.size() / 2);
            if (!cc.compile(ibc + off, len, code)) { ok = false; break; }
            pw::SmallForm f{};
            if (!pw::analyze_small_form(ibc + off, len, f)) { f = pw::SmallForm{}; f.flags = pw::SmallForm::NOT_SMALL; ++not_small; }
            forms.push_back(f);
            xspans.push_back(o);
            xspans.push_back((uint32_t)(code.size() / 2) - o);
        }
    }
    auto up = [&](void** d, const void* h, size_t bytes) {
        if (!device) return true;
        if (hipMalloc(d, bytes ? bytes : 4) != hipSuccess) return false;
        return !bytes || hipMemcpy(*d, h, bytes, hipMemcpyHostToDevice) == hipSuccess;
    };
    std::vector<uint32_t> gstarts{0};
    if (ok) gstarts = pw::logup_group_starts(inter, n_inter, ispans, ibc);
    if (!ok || !up((void**)&p->d_gstarts, gstarts.data(), gstarts.size() * 4) ||
        !up((void**)&p->d_inter, li.data(), li.size() * sizeof(pw::LogupInteraction)) ||
        !up((void**)&p->d_ixspans, xspans.data(), xspans.size() * 4) || !up((void**)&p->d_icode, code.data(), code.size() * 4) ||
        (2 * not_small <= forms.size() && !getenv("POWDR_LOGUP_INTERPRET") &&
         !up((void**)&p->d_iforms, forms.data(), forms.size() * sizeof(pw::SmallForm)))) {
        pw_prover_destroy(p);
        return nullptr;
    }
    p->logup = true;
    p->n_inter = (uint32_t)n_inter;
    p->n_groups = (uint32_t)gstarts.size() - 1;
    p->h_icode = std::move(code);
    p->h_ixspans = std::move(xspans);
    p->h_inter = std::move(li);
    p->h_gstarts = std::move(gstarts);
    return p;
}

extern "C" PwProver* pw_prover_create_logup(const PwStarkConfig* cfg, uint32_t width, const uint32_t* bc, size_t bc_len,
                                            const uint32_t* spans, size_t n_constraints, const uint32_t* inter, size_t n_inter,
                                            const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc, size_t ibc_len) {
    return create_prover_logup(cfg, width, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc, ibc_len, true);
}

// Preprocessed (fixed) columns: the programs name them as operands width .. width + pre_width - 1, so every check of
// the programs runs against the combined bound; the prover then keeps `width` as its main width. At creation the fixed matrix is
// copied behind room for one trace, extended (blow-up 2, shift 31) and committed with the segment tree's own leaf sponge and
// compression — the root is the main commitment a one-AIR segment proof of the fixed matrix would carry.
// the fixed matrix of a prover made with the combined width: kept, extended and committed (NULL: failed, p destroyed)
static PwProver* attach_preprocessed(PwProver* p, uint32_t width, uint32_t pre_width, uint32_t log_height, const uint32_t* d_pre) {
    p->width = width;
    p->pre_width = pre_width;
    p->pre_log_h = log_height;
    const size_t H = (size_t)1 << log_height, N = 2 * H;
    const int L = (int)log_height + 1;
    auto fail = [&]() { (void)hipGetLastError(); pw_prover_destroy(p); return nullptr; };
    (void)hipGetLastError();
    if (poseidon2_upload_params()) return fail();
    CommitLayout Lc{};
    Lc.H = H; Lc.N = N; Lc.panel_cols = lde_panel_cols(H, pre_width);
    if (p->pre_vals.ensure(((size_t)width + pre_width) * H * 4) || p->pre_lde.ensure((size_t)pre_width * N * 4) ||
        p->pre_tree.ensure(merkle_words(N) * 4) || p->coef.ensure(Lc.panel_cols * H * 4) || p->misc.ensure((size_t)pre_width * 8 + 64))
        return fail();
    hipStream_t st = stream();
    uint32_t* fixed = p->pre_vals.as<uint32_t>() + (size_t)width * H;
    if (hipMemcpyAsync(fixed, d_pre, (size_t)pre_width * H * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return fail();
    if (lde_matrix(p, Lc, log_height, fixed, pre_width, p->pre_lde.as<uint32_t>())) return fail();
    std::vector<const uint32_t*> cols(pre_width);
    for (uint32_t c = 0; c < pre_width; ++c) cols[c] = p->pre_lde.as<uint32_t>() + (size_t)c * N;
    const uint32_t** d_cols = p->misc.as<const uint32_t*>();
    if (hipMemcpyAsync(d_cols, cols.data(), cols.size() * 8, hipMemcpyHostToDevice, st) != hipSuccess) return fail();
    std::vector<MixedLevelCols> by_log(L + 1, MixedLevelCols{nullptr, 0});
    by_log[L] = MixedLevelCols{d_cols, pre_width};
    if (merkle_commit_mixed(by_log.data(), L, p->pre_tree.as<uint32_t>(), nullptr)) return fail();
    uint32_t root[8];
    if (hipMemcpyAsync(root, p->pre_tree.as<uint32_t>() + merkle_words(N) - 8, 32, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail();
    for (int k = 0; k < 8; ++k) p->pre_root[k] = bb::from_monty(root[k]);
    return p;
}

extern "C" PwProver* pw_prover_create_preprocessed(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                                   const uint32_t* d_pre, const uint32_t* bc, size_t bc_len, const uint32_t* spans,
                                                   size_t n_constraints, const uint32_t* inter, size_t n_inter, const uint32_t* ispans,
                                                   size_t n_ispans, const uint32_t* ibc, size_t ibc_len) {
    if (!cfg || !width || !pre_width || !d_pre || log_height < 1 || log_height > 26 || (uint64_t)width + pre_width > 0xffffffffull) return nullptr;
    PwProver* p = inter ? create_prover_logup(cfg, width + pre_width, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc, ibc_len, true)
                        : create_prover(cfg, width + pre_width, bc, bc_len, spans, n_constraints, true);
    if (!p) return nullptr;
    return attach_preprocessed(p, width, pre_width, log_height, d_pre);
}

// Next-row operands and row selectors: constraint operands over the row layout of W1 = width + pre_width columns,
// interaction operands below W1, constraint degrees by Plonky3's rule at most 3. pre_width = 0: no fixed matrix (log_height and d_pre
// unused; any height >= 2 rows). A prover whose constraints read only current-row columns acts exactly as the plain (or preprocessed) one.
// device = false: host tables only, no fixed matrix attached (the program checks and the code generation of pw_public_programs_check)
static PwProver* create_row_prover(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height, const uint32_t* d_pre,
                                   uint32_t n_public, const uint32_t* bc, size_t bc_len, const uint32_t* spans, size_t n_constraints,
                                   const uint32_t* inter, size_t n_inter, const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc,
                                   size_t ibc_len, bool device) {
    // (2 W1 + 3 + n_public operands fit in 32 bits)
    if (!cfg || !width || n_public > pw::kMaxPublicValues || (uint64_t)width + pre_width > (n_public ? 0x7fffff00ull : 0x7ffffff0ull)) return nullptr;
    if (device && pre_width && (!d_pre || log_height < 1 || log_height > 26)) return nullptr;
    const uint32_t w1 = width + pre_width;
    PwProver* p = inter ? create_prover_logup(cfg, w1, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc, ibc_len, device, w1, n_public)
                        : create_prover(cfg, w1, bc, bc_len, spans, n_constraints, device, w1, n_public);
    if (!p) return nullptr;
    if (p->max_degree > 3) { pw_prover_destroy(p); return nullptr; }  // a blow-up-2 quotient carries degree 3
    p->transition = true;
    if (!pre_width || !device) { p->width = width; return p; }
    return attach_preprocessed(p, width, pre_width, log_height, d_pre);
}

extern "C" PwProver* pw_prover_create_transition(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                                 const uint32_t* d_pre, const uint32_t* bc, size_t bc_len, const uint32_t* spans,
                                                 size_t n_constraints, const uint32_t* inter, size_t n_inter, const uint32_t* ispans,
                                                 size_t n_ispans, const uint32_t* ibc, size_t ibc_len) {
    return create_row_prover(cfg, width, pre_width, log_height, d_pre, 0, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc,
                             ibc_len, true);
}

// Public values: constraint operands 2 W1 + 3 + k, k < n_public <= 256, of degree 0, behind the row layout. n_public = 0:
// exactly pw_prover_create_transition. The values are set per segment (pw_prover_set_public_values) and never part of the programs.
extern "C" PwProver* pw_prover_create_public(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                             const uint32_t* d_pre, uint32_t n_public, const uint32_t* bc, size_t bc_len, const uint32_t* spans,
                                             size_t n_constraints, const uint32_t* inter, size_t n_inter, const uint32_t* ispans,
                                             size_t n_ispans, const uint32_t* ibc, size_t ibc_len) {
    return create_row_prover(cfg, width, pre_width, log_height, d_pre, n_public, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans,
                             ibc, ibc_len, true);
}

extern "C" uint32_t pw_prover_n_public(const PwProver* p) { return p ? p->n_public : 0; }

// host copy only: a segment proof (and the mock prover) uploads what is set when it begins, on its own launch stream
extern "C" int pw_prover_set_public_values(PwProver* p, const uint32_t* values, size_t n) {
    if (!p || n != p->n_public || (n && !values)) return -1;
    for (size_t k = 0; k < n; ++k) if (values[k] >= bb::P) return -1;
    p->h_pub.resize(n);
    for (size_t k = 0; k < n; ++k) p->h_pub[k] = bb::to_monty(values[k]);
    p->pub_set = true;
    return 0;
}

// Test hook (not declared in include/): what pw_prover_create_public checks and compiles, WITHOUT a GPU — 0 and the highest constraint
// degree, the row flags, the xbc code of the constraints (0 words: the post-fix fallback) and the generated HIP source of all units of
// the specialised quotient kernels, one after the other; -2: the entry would return NULL.
extern "C" int pw_public_programs_check(uint32_t width, uint32_t pre_width, uint32_t n_public, const uint32_t* bc, size_t bc_len,
                                        const uint32_t* spans, size_t n_constraints, const uint32_t* inter, size_t n_inter,
                                        const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc, size_t ibc_len, int* max_degree,
                                        uint32_t* row_flags, uint32_t* xbc_out, size_t xbc_cap, size_t* xbc_len, char* src, size_t src_cap,
                                        size_t* src_len) {
    const PwStarkConfig cfg{1, 0};
    PwProver* p = create_row_prover(&cfg, width, pre_width, 0, nullptr, n_public, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans,
                                    ibc, ibc_len, false);
    if (!p) return -2;
    if (max_degree) *max_degree = p->max_degree;
    if (row_flags) *row_flags = p->row_flags;
    if (xbc_len) *xbc_len = p->h_xcode.size();
    for (size_t i = 0; xbc_out && i < p->h_xcode.size() && i < xbc_cap; ++i) xbc_out[i] = p->h_xcode[i];
    std::string all;
    for (const pw::jit::Unit& u : pw::generate_sources(p, 0, 8000, 8).units) all += u.source;
    if (src_len) *src_len = all.size();
    if (src && src_cap) { strncpy(src, all.c_str(), src_cap - 1); src[src_cap - 1] = 0; }
    pw_prover_destroy(p);
    return 0;
}

extern "C" uint32_t pw_prover_row_flags(const PwProver* p) { return p ? p->row_flags : 0; }
namespace pw {
bool prover_segment_only(const PwProver* p) { return p && (p->pre_width || p->transition || p->n_public); }
}  // namespace pw

extern "C" int pw_prover_preprocessed_root(const PwProver* p, uint32_t* root8) {
    if (!p || !root8 || !p->pre_width) return -1;
    for (int k = 0; k < 8; ++k) root8[k] = p->pre_root[k];
    return 0;
}

extern "C" uint32_t pw_prover_preprocessed_width(const PwProver* p) { return p ? p->pre_width : 0; }

// Code generation + hiprtc compilation of an AIR's specialised kernels WITHOUT a GPU (hiprtc cross-compiles): what
// pw_prover_specialise would build for a prover created from the same tables. interactions == NULL: constraints only.
extern "C" int pw_jit_compile_check(uint32_t width, const uint32_t* bc, size_t bc_len, const uint32_t* spans, size_t n_constraints,
                                    const uint32_t* inter, size_t n_inter, const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc,
                                    size_t ibc_len, size_t* n_kernels, size_t* code_bytes, size_t* n_chunks, char* err, size_t err_cap) {
    const PwStarkConfig cfg{1, 0};
    PwProver* p = inter ? create_prover_logup(&cfg, width, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc, ibc_len, false)
                        : create_prover(&cfg, width, bc, bc_len, spans, n_constraints, false);
    if (!p) return -2;
    const int rc = pw_prover_specialise(p);
    (void)pw_prover_specialised(p, n_kernels, code_bytes, n_chunks);
    if (err && err_cap) { strncpy(err, p->jit.error.c_str(), err_cap - 1); err[err_cap - 1] = 0; }
    pw_prover_destroy(p);
    return rc;
}

// Test hook: the HIP source the code generator emits for translation unit `unit` of an AIR's specialised kernels (which: 0 quotient
// numerator, 1 LogUp permutation columns) under explicit chunking parameters, no compilation. Returns the source's length (0: no such
// unit / the programs did not compile to xbc); buf receives at most cap - 1 characters.
extern "C" size_t pw_jit_generated_source(uint32_t width, const uint32_t* bc, size_t bc_len, const uint32_t* spans, size_t n_constraints,
                                          const uint32_t* inter, size_t n_inter, const uint32_t* ispans, size_t n_ispans, const uint32_t* ibc,
                                          size_t ibc_len, int which, uint32_t chunk_cost, uint32_t chunks_per_unit, size_t unit, char* buf, size_t cap,
                                          char* kernel_name, size_t name_cap, uint32_t* first_chunk, uint32_t* n_chunks, uint32_t* total_chunks) {
    const PwStarkConfig cfg{1, 0};
    PwProver* p = inter ? create_prover_logup(&cfg, width, bc, bc_len, spans, n_constraints, inter, n_inter, ispans, n_ispans, ibc, ibc_len, false)
                        : create_prover(&cfg, width, bc, bc_len, spans, n_constraints, false);
    if (!p) return 0;
    const pw::jit::Generated g = pw::generate_sources(p, which, chunk_cost ? chunk_cost : 8000, chunks_per_unit ? chunks_per_unit : 8);
    pw_prover_destroy(p);
    if (total_chunks) *total_chunks = g.n_chunks;
    if (unit >= g.units.size()) return 0;
    const pw::jit::Unit& u = g.units[unit];
    if (buf && cap) { strncpy(buf, u.source.c_str(), cap - 1); buf[cap - 1] = 0; }
    if (kernel_name && name_cap) { strncpy(kernel_name, u.kernel.c_str(), name_cap - 1); kernel_name[name_cap - 1] = 0; }
    if (first_chunk) *first_chunk = u.first_chunk;
    if (n_chunks) *n_chunks = u.n_chunks;
    return u.source.size();
}

#define TRY(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

extern "C" int pw_prover_logup_path(const PwProver* p) { return !p || !p->logup ? 0 : p->d_iforms ? 2 : 1; }

extern "C" int pw_prover_set_bus_seed(PwProver* p, const uint32_t* seed8) {
    if (!p || !p->logup) return (int)hipErrorInvalidValue;
    p->has_bus_seed = seed8 != nullptr;
    if (seed8) for (int i = 0; i < 8; ++i) p->bus_seed[i] = bb::to_monty(seed8[i] % bb::P);
    return 0;
}

namespace pw {
// (read per call, so that tests can force many small panels: floor 2^12 words, and never fewer than 8 columns)
size_t lde_panel_cols(size_t H, size_t widest) {
    int panel_log_words = 28;
    if (const char* e = getenv("POWDR_PANEL_LOG_WORDS")) { const int v = atoi(e); if (v >= 12 && v <= 32) panel_log_words = v; }
    size_t cols = ((size_t)1 << panel_log_words) / H;
    if (cols < 8) cols = 8;
    if (cols > widest) cols = widest;
    return cols ? cols : 1;
}
int lde_matrix(PwProver* p, const CommitLayout& L, uint32_t log_h, const uint32_t* m, uint32_t cols, uint32_t* out) {
    uint32_t* d_coef = p->coef.as<uint32_t>();
    for (size_t c0 = 0; c0 < cols; c0 += L.panel_cols) {
        const uint32_t pc = (uint32_t)(cols - c0 < L.panel_cols ? cols - c0 : L.panel_cols);
        // Fused schedule (three passes, the coefficient array never touches HBM) where it measured faster than the four-pass
        // one; both read the twiddles of their contiguous stages from tables (profiles/r02_bench_ntt.txt: 1.33x at 2^12 rows —
        // one launch per LDE —, 1.03-1.19x at 2^15..2^20; 0.85-0.98x at 2^13, 2^14, 2^21 and 2^22, where the split of the strided
        // stages is worse); POWDR_LDE_FUSED=0/1 forces one of them.
        const char* ef = getenv("POWDR_LDE_FUSED");
        const bool fused = ef ? atoi(ef) != 0 : (log_h <= 12 || (log_h >= 15 && log_h <= 20));
        if (!fused) {
            TRY(intt_dif(m + c0 * L.H, d_coef, L.H, L.H, pc, (int)log_h));
            TRY(coset_lde_from_coeffs(d_coef, out + c0 * L.N, L.H, L.N, pc, (int)log_h));
        } else {
            TRY(lde_fused(m + c0 * L.H, d_coef, out + c0 * L.N, L.H, L.H, L.N, pc, (int)log_h));
        }
    }
    return 0;
}
}  // namespace pw

namespace {

// ---- streamed proofs ---------------------------------------------------------------------------------------------------
// A proof needs the LDE of every committed column three times: to hash its rows, to evaluate the quotient on them and to answer
// the queries (the DEEP numerator is a polynomial and is extended on its own, see step 4). Resident, that is 8 bytes per committed
// cell next to the caller's trace: BASELINE configs[2] with its bus interactions (3 731 main + 4 632 permutation columns x 2^22
// rows) would need 280 GB. In STREAMED mode (b >= 1) the prover keeps the COEFFICIENTS instead — the trace's in `tcoef`, the
// permutation matrix's in place of the matrix — and walks the extended domain as 2^b sub-cosets (rows r + 2^b i): for each one the
// LDE rows of all columns are rebuilt from the coefficients (ntt.hip subcoset_lde) into `lde`, consumed (leaf hash / quotient
// terms / query rows) and dropped. Same field elements everywhere, hence the same proof words as the resident path
// (tests/test_streamed_prover.py compares both with the oracle).
// Mode: POWDR_STREAM_LOG_BLOCKS = 0 never, b >= 1 always with 2^b sub-cosets (tests); unset: resident when its buffers fit into
// what the device has free (plus what the prover already holds), else the smallest b whose buffers do.
// The DEEP numerator sum_k gamma^k P_k is a polynomial: from 2^16 rows on it is combined on the UN-extended matrices (half the bytes
// the LDE holds) and extended as 4 + 4 columns instead of being accumulated over the LDE of every column (deep_kernel); shorter traces
// keep the one-kernel form (the extra launches cost more than the bytes they save).
// (kDeepComboMinLogHeight: prover_state.hpp; the dispatch is prover_stages.hpp deep_stage, the segment prover's as well)

// consume: the caller hands its trace over (pw_prover_prove_consuming) — a streamed proof then keeps the trace's coefficient arrays IN
// the caller's buffer (no tcoef; what that does to `perm` and `lde`: plan_stage_buffers). To the stage buffers of the AIR the one-AIR
// proof adds its own trees, the trace's coefficient arrays, and in ext_arena / misc everything the proof keeps.
void plan_buffers(const PwProver* p, uint32_t log_h, int b, CommitLayout& L, BufferPlan& B, bool consume = false) {
    const AirShape s = air_shape(p, log_h, p->logup);
    const bool lg = p->logup;
    plan_stage_buffers(p, s, AirMode{b, b && consume}, L, B);
    L.tree_words = merkle_words(s.N);
    L.fri_words = FriLayout(s.logN).fri_words;
    L.n_trees = lg ? 3 : 2;  // trace | quotient | (perm) | FRI
    B.digests = (L.n_trees * L.tree_words + L.fri_words) * 4;
    if (b) { B.tcoef = consume ? 0 : (size_t)s.W * s.H * 4; B.fscale = (size_t)1 << 15; }
    // ext arena: FRI layer vectors v_0 (N) .. v_log_h (2): 2N ext; weights (H); LogUp: second weights, row sums
    B.ext_arena = (2 * s.N + (lg ? 3 : 1) * s.H + s.H / 4096 + 32) * sizeof(bb::Ext);
    const size_t misc_ext = dot_scratch_words(s) + 2 * (size_t)s.K + s.M + p->max_args + 64;  // scratch | opened | gamma powers | alpha, beta powers
    const uint32_t nq = p->cfg.num_queries;
    const size_t path_records = (size_t)nq * (L.n_trees * (size_t)s.logN + (size_t)log_h * s.logN) + 16;
    B.misc = misc_ext * sizeof(bb::Ext) + (size_t)nq * 8 + (size_t)nq * s.K1 * 4 + path_records * (8 + 32) + (size_t)nq * log_h * (8 + 16) + 4096;
}

}  // namespace

namespace pw {
static std::atomic<size_t> g_device_budget{(size_t)-1};  // (size_t)-1: not set yet (POWDR_DEVICE_BUDGET_BYTES is read once); 0: none
size_t device_budget() {
    size_t b = g_device_budget.load();
    if (b == (size_t)-1) {
        const char* e = getenv("POWDR_DEVICE_BUDGET_BYTES");
        b = e ? (size_t)strtoull(e, nullptr, 10) : 0;
        g_device_budget.store(b);
    }
    return b;
}
// What a proof (one AIR's, or a whole segment's) may plan for: buffers are grown by free + malloc, so what the caller's provers hold
// now (`held`) counts as available; 8 % of head room for the allocator's granularity, the twiddle tables and the caller's own small
// allocations during the proof; the device as a whole stays below 90 % (288 GB: 259 GB) — a streamed proof trades a few sub-cosets
// more for room the caller may need between two proofs; and never more than the budget the embedder set (pw_set_device_budget:
// a server that shares the device between several engines). false: the runtime could not say (the caller stays resident).
bool device_room(size_t held, size_t* avail) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
    const size_t others = total_b > free_b + held ? total_b - free_b - held : 0;  // the caller's traces, other provers, the runtime
    size_t a = (size_t)((double)(free_b + held) * 0.92);
    const size_t cap = (size_t)((double)total_b * 0.90);
    a = std::min(a, cap > others ? cap - others : (size_t)0);
    if (const size_t budget = device_budget()) a = std::min(a, budget);
    *avail = a;
    return true;
}
}  // namespace pw

extern "C" void pw_set_device_budget(size_t bytes) { pw::g_device_budget.store(bytes); }
extern "C" size_t pw_get_device_budget(void) { return pw::device_budget(); }

namespace {
// 0 = resident, b >= 1 = streamed over 2^b sub-cosets; < 0: nothing fits
int stream_log_blocks(const PwProver* p, uint32_t log_h, bool consume = false) {
    const int b_max = std::min((int)log_h - 1, 5);  // sub-cosets of at least 4 rows; at most 32 of them (subcoset_lde)
    if (const char* e = getenv("POWDR_STREAM_LOG_BLOCKS")) {
        const int v = atoi(e);
        if (v <= 0 || b_max < 1) return 0;
        return v < b_max ? v : b_max;
    }
    if (log_h < stream_min_log_height()) return 0;  // (a few MB either way)
    size_t avail = 0;
    if (!device_room(pw_prover_device_bytes(p), &avail)) return 0;
    for (int b = 0; b <= b_max; ++b) {
        CommitLayout L;
        BufferPlan B;
        plan_buffers(p, log_h, b, L, B, consume);
        if (B.total() <= avail) return b;
    }
    return -1;
}

int apply_buffers(PwProver* p, const BufferPlan& B) {
    // release before growing: stream_log_blocks counted a held tcoef as available (a consuming proof after a plain streamed one)
    if (!B.tcoef) p->tcoef.release();
    return apply_plan(p, B);
}

// Buffers of the trace commitment, sized as pw_prover_prove needs them (so that a later prove does not reallocate)
int ensure_commit_buffers(PwProver* p, uint32_t log_h, int b, CommitLayout& L) {
    BufferPlan B;
    plan_buffers(p, log_h, b, L, B);
    return apply_buffers(p, B.commit_part());
}

// streamed commitment of a matrix given by its coefficient arrays: every sub-coset's rows are hashed into their leaves
int commit_coefficients(PwProver* p, const CommitLayout& L, uint32_t log_h, const uint32_t* coef, uint32_t cols, uint32_t* d_tree) {
    TRY(streamed::leaf_hashes(stream_ctx(p, air_shape(p, log_h, p->logup), L), coef, cols, d_tree));
    return merkle_build_levels(d_tree, L.N);
}

// LDE + Merkle tree of the trace into p->lde / the first tree of p->digests; root (Montgomery) to the host.
// Streamed: the trace's coefficients into p->tcoef, the tree from the sub-cosets.
int commit_trace(PwProver* p, const CommitLayout& L, const uint32_t* d_trace, uint32_t log_h, uint32_t* root) {
    hipStream_t st = stream();
    uint32_t* d_tdig = p->digests.as<uint32_t>();
    if (L.b) {
        TRY(intt_dif(d_trace, p->tcoef.as<uint32_t>(), L.H, L.H, p->width, (int)log_h));
        TRY(commit_coefficients(p, L, log_h, p->tcoef.as<uint32_t>(), p->width, d_tdig));
    } else {
        TRY(lde_matrix(p, L, log_h, d_trace, p->width, p->lde.as<uint32_t>()));
        TRY(merkle_commit_matrix(p->lde.as<uint32_t>(), L.N, p->width, L.N, d_tdig));
    }
    PW_HIP_TRY(hipMemcpyAsync(root, d_tdig + L.tree_words - 8, 32, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}


}  // namespace

namespace pw {
size_t proof_plan_bytes(const PwProver* p, uint32_t log_h, int b, bool consume) {
    CommitLayout L;
    BufferPlan B;
    plan_buffers(p, log_h, b, L, B, consume && b > 0);
    return B.total();
}
// Every device buffer a proof of a 2^log_h-row trace needs (grown on demand; pw_prover_reserve calls this at set-up
// time so that the first proof does not pay for tens of gigabytes of hipMalloc).
int ensure_proof_buffers(PwProver* p, uint32_t log_h, int b, CommitLayout& L, bool consume) {
    BufferPlan B;
    plan_buffers(p, log_h, b, L, B, consume && b > 0);
    return apply_buffers(p, B);
}
}  // namespace pw

// Trace commitment only (LDE + Merkle root): what a segment's AIRs exchange before the bus seed can be formed.
extern "C" int pw_prover_trace_root(PwProver* p, const uint32_t* d_trace, uint32_t log_h, uint32_t* root8) {
    if (!p || !d_trace || !root8 || log_h < 1 || log_h > 26) return (int)hipErrorInvalidValue;
    if (p->pre_width || p->transition || p->n_public) return -1;  // preprocessed columns, the row layout, public values: segment proofs
    (void)hipGetLastError();
    TRY(poseidon2_upload_params());
    CommitLayout L;
    p->committed_trace = nullptr;
    (void)specialise_provers(&p, 1, &log_h, false);  // before the buffers are sized (the specialised kernels' partial sums)
    const int sb = stream_log_blocks(p, log_h);
    if (sb < 0) return (int)hipErrorOutOfMemory;
    TRY(ensure_commit_buffers(p, log_h, sb, L));
    TRY(commit_trace(p, L, d_trace, log_h, p->committed_root));
    for (int i = 0; i < 8; ++i) root8[i] = bb::from_monty(p->committed_root[i]);
    p->committed_trace = d_trace;
    p->committed_log_h = log_h;
    p->committed_b = sb;
    return (int)hipGetLastError();
}

// The prover's host-mapped landing place for K opened values (PwProver::OpenedMailbox) on the current device, or nullptr (no pinned
// memory to be had, POWDR_OPENINGS_OVERLAP=0): the caller then copies the values after the fact.
static void release_opened_mailbox(PwProver* p) {
    PwProver::OpenedMailbox& mb = p->opened_mb;
    for (int i = 0; i < mb.n_events; ++i) (void)hipEventDestroy(mb.ev[i]);
    mb.n_events = 0;
    if (mb.host) (void)hipHostFree(mb.host);
    mb.host = mb.dev = nullptr;
    mb.cap = 0;
    mb.device = -1;
}

static PwProver::OpenedMailbox* opened_mailbox(PwProver* p, size_t K) {
    const char* env = getenv("POWDR_OPENINGS_OVERLAP");
    if (env && atoi(env) == 0) return nullptr;
    PwProver::OpenedMailbox& mb = p->opened_mb;
    int device = 0;
    if (hipGetDevice(&device) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    if (mb.host && (mb.device != device || mb.cap < K)) release_opened_mailbox(p);
    if (!mb.host) {
        void *h = nullptr, *d = nullptr;
        const size_t cap = std::max<size_t>(K, 64);
        if (hipHostMalloc(&h, cap * sizeof(bb::Ext), hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) { (void)hipGetLastError(); (void)hipHostFree(h); return nullptr; }
        mb.host = (bb::Ext*)h; mb.dev = (bb::Ext*)d; mb.cap = cap; mb.device = device;
        while (mb.n_events < PwProver::OpenedMailbox::kEvents) {
            if (hipEventCreateWithFlags(&mb.ev[mb.n_events], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                release_opened_mailbox(p);
                return nullptr;
            }
            ++mb.n_events;
        }
    }
    return &mb;
}

extern "C" void pw_prover_destroy(PwProver* p) {
    if (!p) return;
    for_each_buffer(p, [](DeviceBuf& b) { b.release(); });
    if (p->d_next_cols) (void)hipFree(p->d_next_cols);
    if (p->d_pub) (void)hipFree(p->d_pub);
    for (void* q : {(void*)p->d_inter, (void*)p->d_ixspans, (void*)p->d_icode, (void*)p->d_gstarts, (void*)p->d_iforms}) if (q) (void)hipFree(q);
    if (p->d_bytecode) (void)hipFree(p->d_bytecode);
    if (p->d_spans) (void)hipFree(p->d_spans);
    release_opened_mailbox(p);
    delete p;
}

extern "C" uint32_t pw_prover_width(const PwProver* p) { return p ? p->width : 0; }
extern "C" int pw_prover_max_constraint_degree(const PwProver* p) { return p ? p->max_degree : -1; }

extern "C" int pw_prover_reserve(PwProver* p, uint32_t log_h) {
    if (!p || log_h < 1 || log_h > 26) return (int)hipErrorInvalidValue;
    (void)hipGetLastError();
    CommitLayout L;
    // the kernels are specialised NOW when the height policy will specialise them at the first proof: their partial-sum buffer is
    // part of the reservation, and the seconds of compilation belong to set-up time as well
    (void)specialise_provers(&p, 1, &log_h, false);
    const int sb = stream_log_blocks(p, log_h);
    if (sb < 0) return (int)hipErrorOutOfMemory;
    return ensure_proof_buffers(p, log_h, sb, L);
}

// 0: the last reservation / proof of a 2^log_height-row trace would keep the LDE resident; b >= 1: it is streamed over 2^b sub-cosets
// (the policy of stream_log_blocks for the CURRENT free memory); -1: not even the streamed buffers fit.
extern "C" int pw_prover_stream_log_blocks(const PwProver* p, uint32_t log_h) {
    if (!p || log_h < 1 || log_h > 26) return -1;
    return stream_log_blocks(p, log_h);
}

extern "C" size_t pw_prover_device_bytes(const PwProver* p) {
    size_t held = 0;
    for_each_buffer(p, [&](const DeviceBuf& b) { held += b.bytes; });
    return held;
}


namespace {
// consume: pw_prover_prove_consuming — d_trace is the caller's to give away. Only a STREAMED proof uses that: the coefficient arrays
// of the trace end up in d_trace itself (no tcoef buffer: 62.6 GB at configs[2], which is what lets it run on 2 sub-cosets instead of 4).
int prove_impl(PwProver* p, const uint32_t* d_trace, uint32_t log_h, const uint32_t** proof_words, size_t* n_words, bool consume) {
    if (!p || !d_trace || log_h < 1 || log_h > 26 || p->pre_width || p->transition || p->n_public) return -1;  // (preprocessed columns, rows: segment proofs only)
    // a handed-over trace becomes a coefficient array that is read 2 / 4 words at a time (fold loads, the DEEP combination)
    if (consume && ((uintptr_t)d_trace & 15)) return (int)hipErrorInvalidValue;
    (void)hipGetLastError();
    const AirShape s = air_shape(p, log_h, p->logup);
    const uint32_t W = s.W, nc = s.nc, n_int = s.n_int, Wp = s.Wp, K1 = s.K1, K = s.K, M = s.M;
    const size_t H = s.H, N = s.N;
    const int logN = s.logN;
    const bool lg = p->logup;
    hipStream_t st = stream();
    TRY(poseidon2_upload_params());
    (void)specialise_provers(&p, 1, &log_h, false);  // run-time specialised expression kernels, compiled once per prover (prover_jit.hip)

    // ---- buffers --------------------------------------------------------------------------
    // digest arena: trace tree | quotient tree | (perm tree) | FRI trees
    // (a consuming proof commits in its own way: a pw_prover_trace_root before it is not reused)
    bool have_commitment = !consume && p->committed_trace == d_trace && p->committed_log_h == log_h;
    p->committed_trace = nullptr;  // one-shot
    // resident LDE, or streamed over 2^sb sub-cosets of the extended domain ("streamed proofs" above)
    int sb = have_commitment ? p->committed_b : stream_log_blocks(p, log_h, consume);
    if (sb < 0) return (int)hipErrorOutOfMemory;
    CommitLayout L;
    int rc_buf = ensure_proof_buffers(p, log_h, sb, L, consume);
    if (rc_buf == (int)hipErrorOutOfMemory && have_commitment && sb == 0) {
        // pw_prove_airs commits every AIR first: several of them may each have chosen "resident" against the same free memory
        // (ADVICE r4). The commitment is dropped and made again in the streamed mode that fits NOW — same root, same words.
        (void)hipGetLastError();
        p->lde.release();
        have_commitment = false;
        sb = stream_log_blocks(p, log_h, false);
        if (sb <= 0) return (int)hipErrorOutOfMemory;
        rc_buf = ensure_proof_buffers(p, log_h, sb, L, false);
    }
    if (rc_buf) return rc_buf;
    const AirMode mode{sb, consume && sb > 0};
    const bool eat = mode.eat;  // the trace is overwritten by its coefficient arrays
    const size_t tree_words = L.tree_words, n_trees = L.n_trees;
    // streamed: the trace's coefficient arrays — in tcoef, or (eat) in the caller's buffer, from the moment nothing reads the trace any more
    uint32_t* d_tcoef = eat ? const_cast<uint32_t*>(d_trace) : p->tcoef.as<uint32_t>();
    const uint32_t nq = p->cfg.num_queries;

    uint32_t* d_lde = p->lde.as<uint32_t>();
    uint32_t* d_dig = p->digests.as<uint32_t>();
    uint32_t* d_qdig = d_dig + tree_words;
    uint32_t* d_pdig = d_dig + 2 * tree_words;          // LogUp only
    uint32_t* d_fdig = d_dig + n_trees * tree_words;
    uint32_t* d_perm = p->perm.as<uint32_t>();
    uint32_t* d_plde = p->plde.as<uint32_t>();
    uint32_t* d_qlde = p->qlde.as<uint32_t>();
    bb::Ext* d_v = p->ext_arena.as<bb::Ext>();          // FRI layers, consecutive
    bb::Ext* d_weights = d_v + 2 * N;
    bb::Ext* d_scratch = p->misc.as<bb::Ext>();
    bb::Ext* d_opened = d_scratch + dot_scratch_words(s);  // K
    bb::Ext* d_gpow = d_opened + K;                        // K
    bb::Ext* d_apow = d_gpow + K;                          // M
    bb::Ext* d_blpow = d_apow + M + 4;                     // max_args + 2
    uint8_t* d_tail = reinterpret_cast<uint8_t*>(d_blpow + p->max_args + 8);
    // trace values | coefficient arrays | alpha, beta powers | weights at zeta, at g zeta (LogUp) | per-row sums, block totals (LogUp) | scratch
    const AirBufs bufs{d_trace, d_trace, d_tcoef, d_apow, d_blpow, d_weights, d_weights + H, d_weights + 2 * H, d_scratch};

    ProofSink pf(p->proof);
    Challenger& ch = pf.ch;
    for (uint32_t x : {lg ? kMagic2 : kMagic, log_h, W, nc}) pf.word(x);
    if (lg) pf.word(n_int);
    for (uint32_t x : {p->cfg.num_queries, p->cfg.pow_bits}) pf.word(x);

    // ---- 1. trace: coefficients, LDE, commitment ---------------------------------------------
    uint32_t root[8];
    // eat + LogUp: the permutation columns are computed from the trace's VALUES after this commitment, so the coefficients go to the
    // (still empty) permutation buffer first; eat without LogUp: nothing reads the values again — in place.
    uint32_t* d_coef_tmp = eat ? (lg ? p->perm.as<uint32_t>() : d_tcoef) : nullptr;
    if (have_commitment) memcpy(root, p->committed_root, 32);  // pw_prover_trace_root already did this step
    else if (eat) {
        TRY(intt_dif(d_trace, d_coef_tmp, H, H, W, (int)log_h));
        TRY(commit_coefficients(p, L, log_h, d_coef_tmp, W, p->digests.as<uint32_t>()));
        PW_HIP_TRY(hipMemcpyAsync(root, p->digests.as<uint32_t>() + tree_words - 8, 32, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
    } else TRY(commit_trace(p, L, d_trace, log_h, root));
    pf.root(root);

    // ---- 1b. LogUp: permutation trace, its LDE and commitment ---------------------------------------
    bb::Ext al = bb::ext_zero(), S = bb::ext_zero();
    if (lg) {
        // the bus challenges come from a transcript that saw only the bus seed (shared by all AIRs of a segment;
        // a lone AIR uses its own trace root), see oracle/stark_oracle.cpp bus_challenges
        uint32_t seed[8];
        memcpy(seed, p->has_bus_seed ? p->bus_seed : root, 32);
        pf.root(seed);
        Challenger cb;
        cb.observe_canonical(kMagic2 % bb::P);
        cb.observe_words(seed, 8);
        al = cb.sample_ext();
        const bb::Ext bl = cb.sample_ext();
        std::vector<bb::Ext> blpow(p->max_args + 2);
        { bb::Ext b = bb::ext_one(); for (auto& x : blpow) { x = b; b = bb::ext_mul(b, bl); } }
        PW_HIP_TRY(hipMemcpyAsync(d_blpow, blpow.data(), blpow.size() * sizeof(bb::Ext), hipMemcpyHostToDevice, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        const uint32_t* s_words[4];  // S = phi(last row)
        TRY(logup_stage(p, s, mode, L, bufs, al, s_words));
        if (sb) TRY(commit_coefficients(p, L, log_h, d_perm, Wp, d_pdig));  // the matrix is its coefficient arrays: sub-coset by sub-coset
        else TRY(merkle_commit_matrix(d_plde, N, Wp, N, d_pdig));
        uint32_t sw[4];
        PW_HIP_TRY(hipMemcpyAsync(root, d_pdig + tree_words - 8, 32, hipMemcpyDeviceToHost, st));
        for (int k = 0; k < 4; ++k) PW_HIP_TRY(hipMemcpyAsync(&sw[k], s_words[k], 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        pf.root(root);
        for (int k = 0; k < 4; ++k) S.c[k] = sw[k];
        pf.ext(S);
    }

    // ---- 2. quotient ---------------------------------------------------------------------------
    const bb::Ext alpha = ch.sample_ext();
    {
        std::vector<bb::Ext> apow(M ? M : 1);
        bb::Ext a = bb::ext_one();
        for (size_t j = M; j-- > 0;) { apow[j] = a; a = bb::ext_mul(a, alpha); }
        if (M) PW_HIP_TRY(hipMemcpyAsync(d_apow, apow.data(), M * sizeof(bb::Ext), hipMemcpyHostToDevice, st));
        PW_HIP_TRY(hipStreamSynchronize(st));  // apow is a stack-local vector
    }
    TRY(quotient_stage(p, s, mode, L, bufs, al, S));
    TRY(merkle_commit_matrix(d_qlde, N, 8, N, d_qdig));
    PW_HIP_TRY(hipMemcpyAsync(root, d_qdig + tree_words - 8, 32, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    pf.root(root);

    // ---- 3. openings at zeta -------------------------------------------------------------------
    const bb::Ext zeta = ch.sample_ext();
    // trace columns: barycentric evaluation straight from the caller's trace (natural order on <g_n>);
    // quotient chunks: from their (small) coefficient arrays
    // internal order of `opened` (= order of the gamma powers): main | perm@zeta | quotient | perm@g*zeta
    const bb::Ext gzeta = bb::ext_scale(zeta, field::root_of_unity((int)log_h));
    // Every matrix's values go straight into host-mapped memory when the prover has it (opened_mailbox), the permutation matrix's in
    // four column slices, with an event after each piece: the host absorbs a piece into the transcript — a sequential sponge, two
    // opened values per permutation — while the device computes the next.
    PwProver::OpenedMailbox* mb = opened_mailbox(p, K);
    bb::Ext* d_open = mb ? mb->dev : d_opened;
    int n_marks = 0;
    auto mark = [&]() -> int {
        if (mb) PW_HIP_TRY(hipEventRecord(mb->ev[n_marks], st));
        ++n_marks;
        return 0;
    };
    const uint32_t n_slices = (mb && Wp >= 1024) ? 4u : 1u;
    uint32_t slice_at[5];
    for (uint32_t i = 0; i <= n_slices; ++i) slice_at[i] = i == n_slices ? Wp : (uint32_t)((uint64_t)Wp * i / n_slices) & ~7u;
    TRY(open_stage(p, s, mode, bufs, zeta, gzeta, d_open, slice_at, n_slices, mark));
    std::vector<bb::Ext> opened_copy;
    const bb::Ext* opened = mb ? mb->host : nullptr;
    if (!mb) {
        opened_copy.resize(K);
        PW_HIP_TRY(hipMemcpyAsync(opened_copy.data(), d_opened, K * sizeof(bb::Ext), hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipStreamSynchronize(st));
        opened = opened_copy.data();
    }
    {
        // proof / transcript order: main, perm@zeta, perm@g*zeta, quotient
        int waited = 0;
        auto wait = [&]() -> int {
            if (mb) PW_HIP_TRY(hipEventSynchronize(mb->ev[waited]));
            ++waited;
            return 0;
        };
        auto emit = [&](size_t a, size_t b) { for (size_t k = a; k < b; ++k) pf.ext(opened[k]); };
        TRY(wait());
        emit(0, W);
        if (lg)
            for (uint32_t i = 0; i < n_slices; ++i) {
                TRY(wait());
                emit((size_t)W + slice_at[i], (size_t)W + slice_at[i + 1]);
            }
        TRY(wait());  // the quotient's values: everything is there
        emit(K1, K);
        emit((size_t)W + Wp, K1);
    }

    // ---- 4. reduced-opening vector -------------------------------------------------------------
    const bb::Ext gamma = ch.sample_ext();
    // the powers of gamma are computed where they are used (CENTRED, the form the DEEP kernels take); the host only needs
    // sum_k gamma^k opened[k] — by Horner's rule, and where the DEEP numerator is combined first (below) while those kernels run
    TRY(gamma_powers(gamma, K, d_gpow));
    bb::Ext opened_sum = bb::ext_zero(), opened_sum2 = bb::ext_zero();
    auto opened_sums = [&]() {
        for (uint32_t k = K1; k-- > 0;) opened_sum = bb::ext_add(bb::ext_mul(opened_sum, gamma), opened[k]);
        for (uint32_t k = K; k-- > K1;) opened_sum2 = bb::ext_add(bb::ext_mul(opened_sum2, gamma), opened[k]);
        opened_sum2 = bb::ext_mul(opened_sum2, bb::ext_pow(gamma, K1));
    };
    TRY(deep_stage(p, s, mode, L, bufs, d_gpow, gamma, opened_sums, opened_sum, opened_sum2, zeta, gzeta, d_v));

    // ---- 5. FRI commit phase --------------------------------------------------------------------
    const FriLayout fri(logN);
    TRY(fri_commit_phase(pf, fri, logN, d_v, d_fdig, bb::to_monty(field::kCosetShift), no_roll_in));  // the coset's shift, squared from round to round

    // ---- 6. proof of work ------------------------------------------------------------------------
    uint32_t witness = 0;
    TRY(grind(ch, p->cfg.pow_bits, reinterpret_cast<uint32_t*>(d_tail), &witness));
    pf.put(witness);

    // ---- 7. queries --------------------------------------------------------------------------------
    if (nq) {
        std::vector<uint32_t> idx(nq);
        for (auto& i : idx) i = ch.sample_bits(logN);
        // layout of the tail buffer
        uint32_t* d_idx = reinterpret_cast<uint32_t*>(d_tail);
        uint32_t* d_loc = d_idx + nq;  // streamed: the queries' rows inside their sub-cosets, sorted by sub-coset
        uint32_t* d_trows = d_loc + nq;
        uint32_t* d_prows = d_trows + (size_t)nq * W;
        uint32_t* d_qrows = d_prows + (size_t)nq * Wp;
        uint64_t* d_offs = reinterpret_cast<uint64_t*>(d_qrows + (size_t)nq * 8 + (((size_t)nq * (K1 + 2)) & 1));
        // digest records (8 words) then FRI sibling records (4 words)
        std::vector<uint64_t> dig_offs, ext_offs;
        for (uint32_t qi = 0; qi < nq; ++qi) {
            const size_t i = idx[qi];
            // proof order: trace path, (perm path), quotient path; arena order: trace | quotient | perm
            for (int tree : {0, 2, 1}) {
                if (tree == 2 && !lg) continue;
                const size_t base = (size_t)tree * tree_words;
                for (int l = 0; l < logN; ++l)
                    dig_offs.push_back(base + merkle_level_offset(N, l) + (((i >> l) ^ 1) * 8));
            }
            fri_query_offsets(i, logN, fri, n_trees * tree_words, ext_offs, dig_offs);
        }
        const size_t n_dig = dig_offs.size(), n_ext = ext_offs.size();
        uint32_t* d_dig_out = reinterpret_cast<uint32_t*>(d_offs + n_dig + n_ext);  // behind the offsets themselves
        uint32_t* d_ext_out = d_dig_out + n_dig * 8;
        PW_HIP_TRY(hipMemcpyAsync(d_idx, idx.data(), nq * 4, hipMemcpyHostToDevice, st));
        if (!sb) {
            TRY(gather_rows(d_lde, N, W, d_idx, nq, d_trows));
            if (lg) TRY(gather_rows(d_plde, N, Wp, d_idx, nq, d_prows));
        } else {
            // streamed: one more pass over the sub-cosets that hold a queried row (prover_stream.hpp query_rows); d_loc and the first nq
            // words of d_qrows (filled afterwards) are its index scratch
            const streamed::Ctx sc = stream_ctx(p, s, L);
            TRY(streamed::query_rows(sc, d_tcoef, W, idx.data(), nq, d_loc, d_qrows, d_trows));
            if (lg) TRY(streamed::query_rows(sc, d_perm, Wp, idx.data(), nq, d_loc, d_qrows, d_prows));
        }
        TRY(gather_rows(d_qlde, N, 8, d_idx, nq, d_qrows));
        // the answers leave the device as canonical words (d_trows .. d_qrows are contiguous); the rows' copies end with the digests'
        TRY(canonicalize_words(d_trows, (size_t)nq * K1));
        std::vector<uint32_t> trows((size_t)nq * W), prows((size_t)nq * Wp + 1), qrows((size_t)nq * 8), dig, ext;
        PW_HIP_TRY(hipMemcpyAsync(trows.data(), d_trows, trows.size() * 4, hipMemcpyDeviceToHost, st));
        if (lg) PW_HIP_TRY(hipMemcpyAsync(prows.data(), d_prows, (size_t)nq * Wp * 4, hipMemcpyDeviceToHost, st));
        PW_HIP_TRY(hipMemcpyAsync(qrows.data(), d_qrows, qrows.size() * 4, hipMemcpyDeviceToHost, st));
        TRY(fetch_query_answers(d_dig, d_v, dig_offs, ext_offs, d_offs, d_dig_out, d_ext_out, 0, [] { return 0; }, dig, ext));
        pf.words.reserve(pf.words.size() + nq + trows.size() + prows.size() + qrows.size() + dig.size() + ext.size());
        size_t dpos = 0, epos = 0;
        for (uint32_t qi = 0; qi < nq; ++qi) {
            pf.put(idx[qi]);
            pf.put_raw(&trows[(size_t)qi * W], W);
            pf.put_raw(&dig[dpos * 8], (size_t)logN * 8); dpos += logN;
            if (lg) {
                pf.put_raw(&prows[(size_t)qi * Wp], Wp);
                pf.put_raw(&dig[dpos * 8], (size_t)logN * 8); dpos += logN;
            }
            pf.put_raw(&qrows[(size_t)qi * 8], 8);
            pf.put_raw(&dig[dpos * 8], (size_t)logN * 8); dpos += logN;
            put_fri_answer(pf, logN, dig, ext, dpos, epos);
        }
    }
    *proof_words = pf.words.data();
    *n_words = pf.words.size();
    return (int)hipGetLastError();
}
}  // namespace

extern "C" int pw_prover_prove(PwProver* p, const uint32_t* d_trace, uint32_t log_h, const uint32_t** proof_words, size_t* n_words) {
    return prove_impl(p, d_trace, log_h, proof_words, n_words, false);
}

// The caller hands the trace over (the reference moves `common_main` into the engine: openvm/src/powdr_extension/trace_generator/
// cuda/mod.rs:415-419). Same proof words. A resident proof leaves the trace as it was; a streamed one leaves its H-scaled coefficient
// arrays in bit-reversed order there (pw_trace_from_coefficients turns them back into the trace).
extern "C" int pw_prover_prove_consuming(PwProver* p, uint32_t* d_trace, uint32_t log_h, const uint32_t** proof_words, size_t* n_words) {
    return prove_impl(p, d_trace, log_h, proof_words, n_words, true);
}

extern "C" int pw_prover_stream_log_blocks_consuming(const PwProver* p, uint32_t log_h) {
    if (!p || log_h < 1 || log_h > 26) return -1;
    return stream_log_blocks(p, log_h, true);
}

// the inverse of what a streamed consuming proof did to the caller's buffer: coefficient arrays (H-scaled, bit-reversed) -> values on <g_n>
extern "C" int pw_trace_from_coefficients(uint32_t* d_coeffs, uint32_t width, uint32_t log_h, uint32_t* d_scratch8k) {
    (void)hipGetLastError();
    if (!d_coeffs || !d_scratch8k || !width || log_h < 1 || log_h > 26) return -1;
    if ((uintptr_t)d_coeffs & 15) return (int)hipErrorInvalidValue;  // the first stage group stages whole tiles with 16-byte loads
    TRY(values_from_coefficients(d_coeffs, d_coeffs, (size_t)1 << log_h, (size_t)1 << log_h, width, (int)log_h, d_scratch8k));
    return (int)hipGetLastError();
}

// ---- mock prover -------------------------------------------------------------------------------------

extern "C" int pw_prover_check_constraints(PwProver* p, const uint32_t* d_trace, uint32_t log_h, uint64_t* n_violations,
                                           uint64_t* first_row, uint32_t* first_constraint) {
    if (!p || !d_trace || log_h > 40 || (p->pre_width && log_h != p->pre_log_h)) return -1;
    if (p->n_public && !p->pub_set) return -1;  // never with zeros in their place
    (void)hipGetLastError();
    if (p->n_public) PW_HIP_TRY(hipMemcpyAsync(p->d_pub, p->h_pub.data(), (size_t)p->n_public * 4, hipMemcpyHostToDevice, stream()));
    const size_t H = (size_t)1 << log_h;
    if (p->row_flags) {
        // the row layout on the trace domain: (trace | fixed) and behind it the next rows (j + 1 mod H) and the
        // selectors' exact values — what the remapped programs read (heights a segment can prove: the roots of unity and the
        // kernel's 32-bit row powers end there)
        if (log_h < 1 || log_h > 26) return -1;
        const uint32_t w1 = p->width + p->pre_width;
        TRY(p->row_vals.ensure(((size_t)w1 + p->row_cols) * H * 4));
        uint32_t* v = p->row_vals.as<uint32_t>();
        PW_HIP_TRY(hipMemcpyAsync(v, d_trace, (size_t)p->width * H * 4, hipMemcpyDeviceToDevice, stream()));
        if (p->pre_width)
            PW_HIP_TRY(hipMemcpyAsync(v + (size_t)p->width * H, p->pre_vals.as<uint32_t>() + (size_t)p->width * H, (size_t)p->pre_width * H * 4,
                                      hipMemcpyDeviceToDevice, stream()));
        TRY(row_layout_columns(v, H, (int)log_h, w1, p->d_next_cols, (uint32_t)p->h_next_cols.size(), 1, (p->row_flags & kRowsSelector) != 0, true));
        d_trace = v;
    } else if (p->pre_width) {  // operands >= width read the fixed matrix: the trace goes in front of it
        PW_HIP_TRY(hipMemcpyAsync(p->pre_vals.as<uint32_t>(), d_trace, (size_t)p->width * H * 4, hipMemcpyDeviceToDevice, stream()));
        d_trace = p->pre_vals.as<uint32_t>();
    }
    TRY(p->misc.ensure(4096));
    unsigned long long* d = p->misc.as<unsigned long long>();
    unsigned long long init[2] = {~0ull, 0ull}, res[2];
    PW_HIP_TRY(hipMemcpyAsync(d, init, sizeof init, hipMemcpyHostToDevice, stream()));
    const ConstraintProgram prog = constraint_program(p, p->n_constraints);
    if (p->n_constraints) TRY(check_constraints(d_trace, H, prog, d));
    PW_HIP_TRY(hipMemcpyAsync(res, d, sizeof res, hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    if (n_violations) *n_violations = res[1];
    if (res[1] && p->n_constraints) {
        if (first_row) *first_row = res[0] / p->n_constraints;
        if (first_constraint) *first_constraint = (uint32_t)(res[0] % p->n_constraints);
    }
    return (int)hipGetLastError();
}

// ---- single stages -----------------------------------------------------------------------------------

extern "C" int pw_lde_batch(const uint32_t* d_trace, uint32_t width, uint32_t log_h, uint32_t* d_coeffs, uint32_t* d_lde) {
    (void)hipGetLastError();
    const size_t H = (size_t)1 << log_h;
    TRY(intt_dif(d_trace, d_coeffs, H, H, width, (int)log_h));
    TRY(coset_lde_from_coeffs(d_coeffs, d_lde, H, 2 * H, width, (int)log_h));
    return (int)hipGetLastError();
}

extern "C" int pw_lde_fused(const uint32_t* d_trace, uint32_t width, uint32_t log_h, uint32_t* d_tmp, uint32_t* d_lde) {
    (void)hipGetLastError();
    const size_t H = (size_t)1 << log_h;
    TRY(lde_fused(d_trace, d_tmp, d_lde, H, H, 2 * H, width, (int)log_h));
    return (int)hipGetLastError();
}

extern "C" int pw_lde_subcoset(const uint32_t* d_coeffs, uint32_t width, uint32_t log_h, uint32_t log_blocks, uint32_t r, uint32_t* d_scale,
                               uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_coeffs || !d_scale || !d_out || !width || log_blocks < 1 || log_blocks > log_h || log_h > 26 || (r >> log_blocks)) return -1;
    if ((uintptr_t)d_coeffs & 15) return (int)hipErrorInvalidValue;  // (16-byte staged loads, as above)
    const size_t H = (size_t)1 << log_h, m = (2 * H) >> log_blocks;
    TRY(subcoset_lde(d_coeffs, d_out, H, m, width, (int)log_h, (int)log_blocks, r, d_scale));
    return (int)hipGetLastError();
}

extern "C" int pw_merkle_commit(const uint32_t* d_matrix, size_t height, uint32_t width, uint32_t* d_digests) {
    (void)hipGetLastError();
    if (!height || (height & (height - 1))) return -1;
    return merkle_commit_matrix(d_matrix, height, width, height, d_digests);
}

// The commitment kernels form by form: each validates its arguments (no launch on a refusal) and forwards to the function of the same
// name in prover_internal.hpp. -1: a malformed argument; hipErrorInvalidValue: a digest / state pointer the uint4 stores cannot take.
static bool misaligned16(const void* p) { return ((uintptr_t)p & 15) != 0; }

extern "C" int pw_merkle_leaf_hash(const uint32_t* d_matrix, size_t height, uint32_t width, size_t col_stride, uint32_t* d_digests,
                                   size_t digest_stride, size_t digest_offset) {
    (void)hipGetLastError();
    if (!d_matrix || !d_digests || !height || !width || col_stride < height || digest_offset >= digest_stride) return -1;
    if (misaligned16(d_digests)) return (int)hipErrorInvalidValue;
    return merkle_leaf_hash(d_matrix, height, width, col_stride, d_digests, digest_stride, digest_offset);
}

extern "C" int pw_merkle_leaf_absorb(const uint32_t* d_matrix, size_t col_stride, const uint32_t* const* d_cols, uint32_t n_cols, uint32_t pos0,
                                     size_t height, size_t row_stride, size_t row_offset, uint32_t* d_state, uint32_t* d_digests, int first,
                                     int last) {
    (void)hipGetLastError();
    if ((d_matrix == nullptr) == (d_cols == nullptr) || !n_cols || pos0 >= 8 || (first && pos0) || !height) return -1;
    if (d_matrix && col_stride < height) return -1;
    if (!row_stride || row_offset >= row_stride) return -1;
    if ((!d_state && !(first && last)) || (last && !d_digests)) return -1;  // the state is read unless `first`, written unless `last`
    if (misaligned16(d_state) || misaligned16(d_digests)) return (int)hipErrorInvalidValue;
    return merkle_leaf_absorb(d_matrix, col_stride, d_cols, n_cols, pos0, height, row_stride, row_offset, d_state, d_digests, first != 0, last != 0);
}

extern "C" int pw_merkle_commit_mixed(const uint32_t* const* d_cols, const uint32_t* n_cols_by_log, const uint32_t* external_by_log, uint32_t L,
                                      uint32_t* d_digests, uint32_t* d_inject) {
    (void)hipGetLastError();
    if (!n_cols_by_log || !external_by_log || !d_digests || L > 27) return -1;
    if (!n_cols_by_log[L] && !external_by_log[L]) return -1;
    MixedLevelCols by_log[28];
    size_t first = 0;
    bool resident = false, below = false;
    for (int k = (int)L; k >= 0; --k) {  // the table holds level k's n_cols_by_log[k] pointers whether the level is external or not
        by_log[k] = MixedLevelCols{d_cols ? d_cols + first : nullptr, n_cols_by_log[k], external_by_log[k]};
        first += n_cols_by_log[k];
        resident = resident || (n_cols_by_log[k] && !external_by_log[k]);
        below = below || (k < (int)L && (n_cols_by_log[k] || external_by_log[k]));
    }
    if ((resident && !d_cols) || (below && !d_inject)) return -1;
    if (misaligned16(d_digests) || misaligned16(d_inject)) return (int)hipErrorInvalidValue;
    return merkle_commit_mixed(by_log, (int)L, d_digests, d_inject);
}

extern "C" int pw_merkle_commit_ext_pairs(const uint32_t* d_values, size_t half, uint32_t* d_digests) {
    (void)hipGetLastError();
    if (!d_values || !d_digests || !half || (half & (half - 1))) return -1;
    if (misaligned16(d_digests)) return (int)hipErrorInvalidValue;
    return merkle_commit_ext_pairs(reinterpret_cast<const bb::Ext*>(d_values), half, d_digests);
}

// ---- the opening, DEEP, FRI, scan and layout kernels, one entry point per function of prover_internal.hpp -------------------
// Thin wrappers: arguments are validated (-1, nothing launched), host scalars converted (canonical -> Montgomery), the internal
// function's own refusals passed through. No kernel code lives here. Launches go to stream() and are not waited for, except by
// the two calls that own scratch (StageScratch below).
namespace {

constexpr uint32_t kStageMaxLog = 27;  // the field's two-adicity: field::root_of_unity and the kernels' 32-bit row powers end here

// 4 canonical host words -> Ext; false: a NULL pointer or a word >= p
bool stage_ext(const uint32_t* c4, bb::Ext* out) {
    if (!c4) return false;
    for (int k = 0; k < 4; ++k) {
        if (c4[k] >= bb::P) return false;
        out->c[k] = bb::to_monty(c4[k]);
    }
    return true;
}

// scratch of one stage call: released when the call returns, after the launch stream has drained (the kernels still read it)
struct StageScratch {
    void* p = nullptr;
    int alloc(size_t bytes) { return (int)hipMalloc(&p, bytes ? bytes : 4); }
    template <class T> T* as() const { return static_cast<T*>(p); }
    ~StageScratch() {
        if (!p) return;
        (void)hipStreamSynchronize(stream());
        (void)hipFree(p);
    }
};

}  // namespace

extern "C" int pw_stage_opening_weights(const uint32_t* zeta, uint32_t log_h, int on_coefficients, uint32_t* d_w) {
    (void)hipGetLastError();
    bb::Ext z;
    if (!stage_ext(zeta, &z) || !d_w || log_h > kStageMaxLog - 1) return -1;
    return on_coefficients ? zeta_weights(z, (int)log_h, reinterpret_cast<bb::Ext*>(d_w))
                           : barycentric_weights(z, (int)log_h, reinterpret_cast<bb::Ext*>(d_w));
}

extern "C" int pw_stage_ext_dot(const uint32_t* d_cols, size_t stride, uint32_t n_cols, size_t len, const uint32_t* d_w, const uint32_t* d_w2,
                                uint32_t* d_out, uint32_t* d_out2) {
    (void)hipGetLastError();
    if (!d_cols || !d_w || !d_out || (d_w2 && !d_out2) || !n_cols || !len || stride < len) return -1;
    if (misaligned16(d_w) || misaligned16(d_w2)) return (int)hipErrorInvalidValue;  // (the kernel loads a weight as one uint4)
    const size_t n_chunks = (len + 8191) / 8192;  // (ext_dot_columns2's scratch, prover_internal.hpp)
    StageScratch s;
    TRY(s.alloc((d_w2 ? 2 : 1) * (size_t)n_cols * n_chunks * sizeof(bb::Ext)));
    const bb::Ext* w = reinterpret_cast<const bb::Ext*>(d_w);
    if (!d_w2) return ext_dot_columns(d_cols, stride, n_cols, len, w, reinterpret_cast<bb::Ext*>(d_out), s.as<bb::Ext>());
    return ext_dot_columns2(d_cols, stride, n_cols, len, w, reinterpret_cast<const bb::Ext*>(d_w2), reinterpret_cast<bb::Ext*>(d_out),
                            reinterpret_cast<bb::Ext*>(d_out2), s.as<bb::Ext>());
}

extern "C" int pw_stage_ext_powers(const uint32_t* base, uint32_t n, int reversed, int centred, uint32_t* d_out) {
    (void)hipGetLastError();
    bb::Ext b;
    if (!stage_ext(base, &b) || !d_out) return -1;
    return ext_powers(b, n, reversed != 0, centred != 0, reinterpret_cast<bb::Ext*>(d_out));
}

extern "C" int pw_stage_deep(const uint32_t* d_a, uint32_t wa, const uint32_t* d_b, uint32_t wb, uint32_t log_n, const uint32_t* d_gpow,
                             const uint32_t* sum, const uint32_t* zeta, uint32_t* d_v) {
    (void)hipGetLastError();
    bb::Ext s, z;
    if (!stage_ext(sum, &s) || !stage_ext(zeta, &z) || !d_gpow || !d_v || (wa && !d_a) || (wb && !d_b) || !(wa | wb)) return -1;
    if (log_n < 1 || log_n > kStageMaxLog) return -1;
    return deep_quotient(d_a, wa, d_b, wb, (size_t)1 << log_n, (int)log_n, reinterpret_cast<const bb::Ext*>(d_gpow), s, z,
                         reinterpret_cast<bb::Ext*>(d_v));
}

extern "C" int pw_stage_deep_logup(const uint32_t* d_lde, uint32_t W, const uint32_t* d_plde, uint32_t Wp, const uint32_t* d_qlde, uint32_t log_n,
                                   const uint32_t* d_gpow, const uint32_t* gK, const uint32_t* sum1, const uint32_t* sum2, const uint32_t* zeta,
                                   const uint32_t* gzeta, uint32_t* d_v) {
    (void)hipGetLastError();
    bb::Ext s1, s2, z, gz, k = bb::ext_zero();
    if (!stage_ext(sum1, &s1) || !stage_ext(sum2, &s2) || !stage_ext(zeta, &z) || !stage_ext(gzeta, &gz) || (gK && !stage_ext(gK, &k))) return -1;
    if (!d_gpow || !d_qlde || !d_v || (W && !d_lde) || (Wp && !d_plde)) return -1;
    if (log_n < 1 || log_n > kStageMaxLog) return -1;
    const size_t N = (size_t)1 << log_n;
    const bb::Ext* g = reinterpret_cast<const bb::Ext*>(d_gpow);
    bb::Ext* v = reinterpret_cast<bb::Ext*>(d_v);
    return gK ? deep_quotient_two_point(d_lde, W, d_plde, Wp, d_qlde, N, (int)log_n, g, k, s1, s2, z, gz, v)
              : deep_quotient_logup(d_lde, W, d_plde, Wp, d_qlde, N, (int)log_n, g, s1, s2, z, gz, v);
}

extern "C" int pw_stage_ext_lincomb(const uint32_t* d_a, uint32_t wa, const uint32_t* d_b, uint32_t wb, size_t len, const uint32_t* d_gpow,
                                    uint32_t second, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_gpow || !d_out || (wa && !d_a) || (wb && !d_b) || !(wa | wb) || !len) return -1;
    return ext_lincomb(d_a, wa, d_b, wb, len, reinterpret_cast<const bb::Ext*>(d_gpow), second, d_out);
}

extern "C" int pw_stage_deep_from_combo(const uint32_t* d_glde, const uint32_t* d_qlde, uint32_t log_n, const uint32_t* d_gq, const uint32_t* sum1,
                                        const uint32_t* sum2, const uint32_t* zeta, const uint32_t* gzeta, int two, uint32_t* d_v) {
    (void)hipGetLastError();
    bb::Ext s1, s2, z, gz;
    if (!stage_ext(sum1, &s1) || !stage_ext(sum2, &s2) || !stage_ext(zeta, &z) || !stage_ext(gzeta, &gz)) return -1;
    if (!d_glde || !d_qlde || !d_gq || !d_v || log_n < 1 || log_n > kStageMaxLog) return -1;
    return deep_from_combo(d_glde, d_qlde, (size_t)1 << log_n, (int)log_n, reinterpret_cast<const bb::Ext*>(d_gq), s1, s2, z, gz, two != 0,
                           reinterpret_cast<bb::Ext*>(d_v));
}

extern "C" int pw_stage_fri_fold(const uint32_t* d_v, uint32_t log_size, uint32_t shift, const uint32_t* beta, uint32_t* d_out) {
    (void)hipGetLastError();
    bb::Ext b;
    if (!stage_ext(beta, &b) || !d_v || !d_out || log_size < 1 || log_size > kStageMaxLog || !shift || shift >= bb::P) return -1;
    return fri_fold(reinterpret_cast<const bb::Ext*>(d_v), (size_t)1 << (log_size - 1), (int)log_size, bb::to_monty(shift), b,
                    reinterpret_cast<bb::Ext*>(d_out));
}

extern "C" int pw_stage_logup_scan(const uint32_t* d_rowsum, size_t H, uint32_t* d_phi_cols) {
    (void)hipGetLastError();
    if (!d_rowsum || !d_phi_cols || !H || H > ((size_t)1 << kStageMaxLog)) return -1;
    StageScratch s;
    TRY(s.alloc((H / 4096 + 1) * sizeof(bb::Ext)));  // (logup_perm_trace's d_block_totals, prover_internal.hpp)
    return logup_scan(reinterpret_cast<const bb::Ext*>(d_rowsum), H, s.as<bb::Ext>(), d_phi_cols);
}

extern "C" int pw_stage_quotient_split(const uint32_t* d_cbr, uint32_t log_h, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_cbr || !d_out || log_h > kStageMaxLog - 1) return -1;
    if ((uintptr_t)d_cbr & 7) return (int)hipErrorInvalidValue;  // (the kernel loads a pair of rows as one uint2)
    return quotient_split(d_cbr, (size_t)1 << log_h, (int)log_h, d_out);
}

extern "C" int pw_stage_row_layout(uint32_t* d_m, uint32_t log_n, uint32_t w1, const uint32_t* d_next_cols, uint32_t n_next, uint32_t step,
                                   int selectors, int trace_domain) {
    (void)hipGetLastError();
    if (!d_m || (n_next && !d_next_cols) || log_n < 1 || log_n > kStageMaxLog) return -1;
    return row_layout_columns(d_m, (size_t)1 << log_n, (int)log_n, w1, d_next_cols, n_next, step, selectors != 0, trace_domain != 0);
}

extern "C" int pw_stage_part_scatter(const uint32_t* d_part, uint32_t n_chunks, size_t m, uint32_t b, uint32_t r, size_t N, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_part || !d_out || !n_chunks || !m || b > kStageMaxLog || (r >> b)) return -1;
    if (m > (N >> b) || r + ((m - 1) << b) >= N) return -1;  // the last row written, r + 2^b (m - 1), lies inside the N-row vector
    return part_scatter(d_part, n_chunks, m, (int)b, r, N, d_out);
}

extern "C" int pw_stage_ext_axpy(uint32_t* d_y, const uint32_t* a, const uint32_t* d_x, size_t n) {
    (void)hipGetLastError();
    bb::Ext e;
    if (!d_y || !d_x || !n || (a && !stage_ext(a, &e))) return -1;
    return ext_axpy(reinterpret_cast<bb::Ext*>(d_y), a ? &e : nullptr, reinterpret_cast<const bb::Ext*>(d_x), n);
}

// ---- the LogUp permutation and quotient stages of one prover --------------------------------------------------------------------
// They take the prover because the programs live there, and run the path that prover would run: the specialised kernels if it has
// them, else the interpreter (small forms, or post-fix where the prover was created so). The challenge TABLES are the caller's.
namespace {

// a prover these calls serve: no preprocessed columns, no row layout, no public values (whole proofs cover those)
bool stage_prover(const PwProver* p) { return p && !p->pre_width && !p->row_flags && !p->n_public && !p->transition; }

// the partial sums quotient_eval combines for nc constraints on `rows` rows (its own rounding of quotient_chunks)
uint32_t quotient_eval_chunks(size_t rows, uint32_t nc) {
    const uint32_t chunks = quotient_chunks(rows, nc);
    if (chunks <= 1) return 1;
    const uint32_t per_chunk = (nc + chunks - 1) / chunks;
    return (nc + per_chunk - 1) / per_chunk;
}

}  // namespace

extern "C" int pw_stage_logup_perm(PwProver* p, const uint32_t* d_values, uint32_t log_h, const uint32_t* alpha, const uint32_t* d_blpow,
                                   uint32_t* d_perm, uint32_t* d_rowsum) {
    (void)hipGetLastError();
    bb::Ext al;
    if (!stage_prover(p) || !p->logup || !stage_ext(alpha, &al) || !d_values || !d_blpow || !d_perm || !d_rowsum || log_h > kStageMaxLog - 1) return -1;
    const size_t H = (size_t)1 << log_h;
    StageScratch s;
    TRY(s.alloc((H / 4096 + 1) * sizeof(bb::Ext)));  // (logup_perm_trace's d_block_totals, prover_internal.hpp)
    const bb::Ext* bl = reinterpret_cast<const bb::Ext*>(d_blpow);
    bb::Ext* rowsum = reinterpret_cast<bb::Ext*>(d_rowsum);
    if (specialised(p)) return logup_perm_trace_jit(p, d_values, H, al, bl, d_perm, rowsum, s.as<bb::Ext>());
    return logup_perm_trace(d_values, H, logup_program(p, air_shape(p, log_h, true)), al, bl, d_perm, rowsum, s.as<bb::Ext>());
}

extern "C" int pw_stage_quotient(PwProver* p, const uint32_t* d_lde, const uint32_t* d_plde, uint32_t log_n, const uint32_t* d_apow,
                                 const uint32_t* alpha, const uint32_t* d_blpow, const uint32_t* S, uint32_t* d_q, uint32_t* n_chunks_out) {
    (void)hipGetLastError();
    if (!stage_prover(p) || !d_lde || !d_apow || !d_q || log_n < 1 || log_n > kStageMaxLog) return -1;
    const bool lg = p->logup, jit = specialised(p);
    bb::Ext al = bb::ext_zero(), sum = bb::ext_zero();
    if (lg ? (!d_plde || !d_blpow || !stage_ext(alpha, &al) || !stage_ext(S, &sum)) : (d_plde || d_blpow || alpha || S)) return -1;
    const size_t N = (size_t)1 << log_n;
    const uint32_t nc = p->n_constraints;
    uint32_t zv_even, zv_odd;
    vanishing_on_coset(log_n - 1, &zv_even, &zv_odd);
    const bb::Ext* apow = reinterpret_cast<const bb::Ext*>(d_apow);
    const bb::Ext* bl = reinterpret_cast<const bb::Ext*>(d_blpow);
    const ConstraintProgram prog = constraint_program(p, nc);
    uint32_t chunks = 1;
    int rc;
    if (lg && jit) {
        chunks = p->jit.quotient.n_chunks;
        rc = quotient_eval_logup_jit(p, d_lde, d_plde, N, (int)log_n, apow, al, bl, sum, zv_even, zv_odd, d_q);
    } else if (lg) {
        rc = quotient_eval_logup(d_lde, d_plde, N, (int)log_n, prog, logup_program(p, air_shape(p, log_n - 1, true)), apow, al, bl, sum, zv_even, zv_odd, d_q);
    } else if (jit && nc) {
        chunks = p->jit.quotient.n_chunks;
        rc = quotient_eval_jit(p, d_lde, N, apow, bb::inv(zv_even), bb::inv(zv_odd), d_q);
    } else {
        chunks = quotient_eval_chunks(N, nc);
        StageScratch s;
        TRY(s.alloc(chunks > 1 ? (size_t)chunks * 4 * N * 4 : 0));
        rc = quotient_eval(d_lde, N, prog, apow, bb::inv(zv_even), bb::inv(zv_odd), d_q, chunks > 1 ? s.as<uint32_t>() : nullptr, chunks);
    }
    if (!rc && n_chunks_out) *n_chunks_out = chunks;
    return rc;
}

extern "C" uint32_t pw_prover_quotient_units(const PwProver* p) { return p && specialised(p) ? quotient_units_jit(p) : 0u; }

extern "C" int pw_prover_quotient_unit_groups(const PwProver* p, uint32_t unit, uint32_t* g0, uint32_t* g1) {
    if (!p || !g0 || !g1 || !specialised(p) || unit >= quotient_units_jit(p)) return -1;
    quotient_unit_groups(p, unit, g0, g1);
    return 0;
}

extern "C" int pw_stage_quotient_sums(PwProver* p, const uint32_t* d_T, const uint32_t* d_Pm, size_t rows, uint32_t log_n, const uint32_t* d_apow,
                                      const uint32_t* alpha, const uint32_t* d_blpow, int unit, uint32_t* d_part, uint32_t* n_parts_out) {
    (void)hipGetLastError();
    if (!stage_prover(p) || !d_T || !d_apow || !d_part || !rows || rows > ((size_t)1 << kStageMaxLog) || log_n < 1 || log_n > kStageMaxLog) return -1;
    const bool lg = p->logup, jit = specialised(p);
    bb::Ext al = bb::ext_zero();
    if (lg ? (!d_Pm || !d_blpow || !stage_ext(alpha, &al)) : (d_Pm || d_blpow || alpha)) return -1;
    if (unit >= 0 && (!jit || (uint32_t)unit >= quotient_units_jit(p))) return -1;
    const uint32_t nc = p->n_constraints, one = bb::R_MOD_P;
    const bb::Ext* apow = reinterpret_cast<const bb::Ext*>(d_apow);
    const bb::Ext* bl = reinterpret_cast<const bb::Ext*>(d_blpow);
    const ConstraintProgram prog = constraint_program(p, nc);
    uint32_t n_parts = 1;
    int rc;
    if (unit >= 0) {
        uint32_t g0 = 0, g1 = 0;
        quotient_unit_groups(p, (uint32_t)unit, &g0, &g1);
        n_parts = p->jit.quotient.n_chunks;
        rc = quotient_unit_jit(p, (uint32_t)unit, d_T, lg ? streamed::unit_panel_origin(d_Pm, g0, rows) : nullptr, rows, apow, al, bl, d_part);
    } else if (jit && (nc || lg)) {
        rc = quotient_parts_jit(p, d_T, d_Pm, rows, apow, al, bl, d_part, &n_parts);
    } else if (lg) {
        rc = quotient_eval_logup(d_T, d_Pm, rows, (int)log_n, prog, logup_program(p, air_shape(p, log_n - 1, true)), apow, al, bl, bb::ext_zero(), one, one,
                                 d_part, true);
    } else {
        const uint32_t chunks = quotient_eval_chunks(rows, nc);
        StageScratch s;
        TRY(s.alloc(chunks > 1 ? (size_t)chunks * 4 * rows * 4 : 0));
        rc = quotient_eval(d_T, rows, prog, apow, one, one, d_part, chunks > 1 ? s.as<uint32_t>() : nullptr, chunks);
    }
    if (!rc && n_parts_out) *n_parts_out = n_parts;
    return rc;
}

extern "C" int pw_stage_logup_tail(const uint32_t* d_part, uint32_t n_chunks, const uint32_t* d_plde_phi, const uint32_t* d_plde_sumq, uint32_t log_n,
                                   const uint32_t* d_apow_tail, const uint32_t* S, uint32_t* d_q) {
    (void)hipGetLastError();
    bb::Ext sum;
    if (!d_part || !n_chunks || !d_plde_phi || !d_plde_sumq || !d_apow_tail || !d_q || !stage_ext(S, &sum) || log_n < 1 || log_n > kStageMaxLog) return -1;
    uint32_t zv_even, zv_odd;
    vanishing_on_coset(log_n - 1, &zv_even, &zv_odd);
    return quotient_logup_tail(d_part, n_chunks, d_plde_phi, d_plde_sumq, (size_t)1 << log_n, (int)log_n, reinterpret_cast<const bb::Ext*>(d_apow_tail), sum,
                               zv_even, zv_odd, d_q);
}

extern "C" int pw_stage_rowsum_combine(const uint32_t* d_part, uint32_t n_chunks, size_t H, uint32_t* d_rowsum, uint32_t* d_cols4) {
    (void)hipGetLastError();
    if (!d_part || !n_chunks || !d_rowsum || !d_cols4 || !H || H > ((size_t)1 << kStageMaxLog)) return -1;
    return logup_rowsum_combine(d_part, n_chunks, H, reinterpret_cast<bb::Ext*>(d_rowsum), d_cols4);
}

// ---- the query phase: grinding, the gathers, a streamed AIR's rows -------------------------------------------------------------
// The same thin wrappers: each forwards to the function the provers call (grind_search, gather_rows, gather_rows_multi, gather_records,
// gather_words, canonicalize_words, ext_to_cols, streamed::query_rows_core).
static_assert(sizeof(PwStageGatherJob) == sizeof(GatherRowsJob), "PwStageGatherJob restates GatherRowsJob");

extern "C" int pw_stage_pow_grind(const uint32_t* state16, const uint32_t* pending, uint32_t in_len, uint32_t bits, uint32_t* witness_out) {
    (void)hipGetLastError();
    // bits: the provers hand any non-zero pow_bits to the search (0 = no proof of work), and a sampled word has 31 bits (1u << bits)
    if (!state16 || !witness_out || (in_len && !pending) || in_len > 7 || bits < 1 || bits > 31) return -1;
    uint32_t st[16], in[8] = {0};
    for (int i = 0; i < 16; ++i) { if (state16[i] >= bb::P) return -1; st[i] = bb::to_monty(state16[i]); }
    for (uint32_t i = 0; i < in_len; ++i) { if (pending[i] >= bb::P) return -1; in[i] = bb::to_monty(pending[i]); }
    StageScratch s;
    TRY(s.alloc(25 * 4));
    return grind_search(st, in, in_len, bits, s.as<uint32_t>(), witness_out);
}

extern "C" int pw_stage_canonicalize(uint32_t* d_words, size_t n) {
    (void)hipGetLastError();
    if (!d_words || !n) return -1;
    return canonicalize_words(d_words, n);
}

extern "C" int pw_stage_gather_rows(const uint32_t* d_m, size_t height, uint32_t width, const uint32_t* d_idx, uint32_t n_idx, int canonical,
                                    uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_m || !d_idx || !d_out || !height || !width || !n_idx || n_idx > 65535u) return -1;  // (blockIdx.y is the query)
    TRY(gather_rows(d_m, height, width, d_idx, n_idx, d_out));
    return canonical ? canonicalize_words(d_out, (size_t)n_idx * width) : 0;
}

extern "C" int pw_stage_gather_rows_multi(const PwStageGatherJob* jobs, uint32_t n_jobs, const uint32_t* d_idx, uint32_t n_idx, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!jobs || !d_idx || !d_out || !n_jobs || !n_idx || n_jobs > 65535u || n_idx > 65535u) return -1;
    std::vector<GatherRowsJob> h(n_jobs);
    for (uint32_t k = 0; k < n_jobs; ++k) {
        if (!jobs[k].d_m || !jobs[k].height || !jobs[k].width) return -1;
        h[k] = GatherRowsJob{jobs[k].d_m, jobs[k].height, jobs[k].width, jobs[k].idx_off, jobs[k].out_off};
    }
    StageScratch s;
    TRY(s.alloc(h.size() * sizeof(GatherRowsJob)));
    PW_HIP_TRY(hipMemcpyAsync(s.p, h.data(), h.size() * sizeof(GatherRowsJob), hipMemcpyHostToDevice, stream()));
    return gather_rows_multi(s.as<GatherRowsJob>(), n_jobs, gather_rows_max_width(h.data(), h.size()), d_idx, n_idx, d_out);
}

extern "C" int pw_stage_gather_records(const uint32_t* d_arena, const uint64_t* offsets, uint32_t words_per_record, uint32_t n, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_arena || !offsets || !d_out || !words_per_record || !n || (uint64_t)n * words_per_record > 0xffffffffull) return -1;
    StageScratch s;
    TRY(s.alloc((size_t)n * 8));
    PW_HIP_TRY(hipMemcpyAsync(s.p, offsets, (size_t)n * 8, hipMemcpyHostToDevice, stream()));
    return gather_records(d_arena, s.as<uint64_t>(), words_per_record, n, d_out);
}

extern "C" int pw_stage_gather_words(const uint32_t* const* d_ptrs, uint32_t n, uint32_t* d_out) {
    (void)hipGetLastError();
    if (!d_ptrs || !d_out || !n) return -1;
    return gather_words(d_ptrs, n, d_out);
}

extern "C" int pw_stage_ext_to_cols(const uint32_t* d_in, size_t len, uint32_t* d_cols4) {
    (void)hipGetLastError();
    if (!d_in || !d_cols4 || !len || len > ((size_t)1 << kStageMaxLog)) return -1;
    return ext_to_cols(reinterpret_cast<const bb::Ext*>(d_in), len, d_cols4);
}

extern "C" int pw_stage_query_rows(const uint32_t* d_coeffs, uint32_t cols, uint32_t log_h, uint32_t log_blocks, const uint32_t* idx, uint32_t n_idx,
                                   uint32_t* d_work, size_t work_words, size_t select_words, uint32_t* d_scale, uint32_t* d_rows, uint8_t* forms) {
    (void)hipGetLastError();
    if (!d_coeffs || !idx || !d_work || !d_scale || !d_rows || !cols || !n_idx || n_idx > 65535u) return -1;
    if (log_blocks < 1 || log_blocks > 5 || log_blocks > log_h || log_h > 26) return -1;  // (pw_lde_subcoset's range; subcoset_spec: b <= 5)
    const size_t H = (size_t)1 << log_h, m = (2 * H) >> log_blocks;
    for (uint32_t q = 0; q < n_idx; ++q) if (idx[q] >= 2 * H) return -1;
    if (work_words < (size_t)cols * m || select_words > work_words) return -1;
    if (((uintptr_t)d_coeffs & 15) || ((uintptr_t)d_work & 7)) return (int)hipErrorInvalidValue;  // (16-byte staged loads; the 64-bit sums)
    StageScratch s;
    TRY(s.alloc((size_t)n_idx * 8));
    uint32_t* d_loc = s.as<uint32_t>();
    return streamed::query_rows_core(d_coeffs, cols, log_h, (int)log_blocks, idx, n_idx, d_loc, d_loc + n_idx, d_rows, d_work, select_words, d_scale,
                                     forms);
}

extern "C" int pw_set_poseidon2_constants(const uint32_t* ext_rc, const uint32_t* int_rc) {
    return poseidon2_set_constants(ext_rc, int_rc);
}

extern "C" void pw_get_poseidon2_constants(uint32_t* ext_rc, uint32_t* int_rc, uint32_t* diag) {
    const p2::Params& p = poseidon2_params_host();
    if (ext_rc) for (int r = 0; r < 8; ++r) for (int i = 0; i < 16; ++i) ext_rc[16 * r + i] = bb::from_monty(p.ext_rc[r][i]);
    if (int_rc) for (int r = 0; r < 13; ++r) int_rc[r] = bb::from_monty(p.int_rc[r]);
    if (diag) for (int i = 0; i < 16; ++i) diag[i] = bb::from_monty(p.diag[i]);
}

extern "C" void pw_poseidon2_permute_host(uint32_t* s) {
    uint32_t m[16];
    for (int i = 0; i < 16; ++i) m[i] = bb::to_monty(s[i] % bb::P);
    p2::permute(m, poseidon2_params_host());
    for (int i = 0; i < 16; ++i) s[i] = bb::from_monty(m[i]);
}
