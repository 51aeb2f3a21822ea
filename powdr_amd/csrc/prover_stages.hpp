// What is done to ONE AIR between two commitments, shared by the one-AIR prover (prover.hip: pw-stark v0) and the segment prover
// (segment_prover.hip: v1): the shape numbers, the plan of the per-AIR stage buffers, and the stages themselves — LogUp permutation
// matrix, quotient, openings, DEEP numerator, proof of work — and what the two protocols do alike around them: the proof sink (words +
// transcript), the FRI commit phase, fetching the query answers and emitting their FRI part. The protocols differ in the header, in how
// commitments and the trees' query answers are laid out, and in what FRI folds (a shifted coset; unshifted subgroups with the smaller
// heights rolled in): that stays with the callers. What they
// place differently (trace values, coefficient arrays, power tables, weights, scratch, outputs) comes in as pointers; the stage
// buffers proper are the prover object's (perm, plde, q, qpart, qcoef, qlde, gbuf; lde for the resident LDE or one sub-coset).
// Every stage enqueues on pw::stream() as it is at the time of the call (the segment prover moves it from AIR to AIR) and none
// synchronises with the host (the FRI commit phase and fetch_query_answers do, and say so). The streamed arms are prover_stream.hpp's. Not part of the C ABI.
#pragma once
#include "prover_stream.hpp"
#include "logup_groups.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace pw {

#define PW_STRY(x) do { const int _rc = (x); if (_rc) return _rc; } while (0)

struct AirShape {
    uint32_t W, nc, n_int, n_g, log_h;
    uint32_t Wp;      // permutation matrix: q_g coordinates per group, then phi (0 without LogUp)
    uint32_t M;       // folded constraints
    uint32_t Wf, W1;  // preprocessed columns, W1 = W + Wf: the columns the programs and the zeta openings see
    // the row layout: rf = kRowsNext | kRowsSelector (0: not row-aware), Wr = the values behind the W1 columns of the
    // LDE (next rows, selectors), Wg = the columns opened at g zeta besides the permutation matrix (W1 for a two-point AIR, else 0)
    uint32_t rf, Wr, Wg;
    uint32_t K1, K;   // polynomials opened at zeta: main | preprocessed | perm | quotient; K = K1 + those opened at g zeta (perm | Wg)
    size_t H, N;
    int logN;
};

// logup: the proof carries the LogUp extension (a prover made with interactions may serve a constraints-only segment)
inline AirShape air_shape(const PwProver* p, uint32_t log_h, bool logup) {
    AirShape s{};
    s.W = p->width; s.nc = p->n_constraints; s.log_h = log_h;
    s.n_int = logup ? p->n_inter : 0; s.n_g = logup ? p->n_groups : 0; s.Wp = logup ? 4 * (s.n_g + 1) : 0;
    s.M = s.nc + (logup ? s.n_g + 3 : 0);
    s.Wf = p->pre_width; s.W1 = s.W + s.Wf;
    s.rf = p->row_flags; s.Wr = p->row_cols; s.Wg = (s.rf & kRowsNext) ? s.W1 : 0;
    s.K1 = s.W1 + s.Wp + 8;
    s.K = s.K1 + s.Wp + s.Wg;
    s.H = (size_t)1 << log_h; s.N = 2 * s.H; s.logN = (int)log_h + 1;
    return s;
}

struct AirMode {
    int b;     // the extended domain is walked as 2^b sub-cosets (0: the LDE is resident)
    bool eat;  // streamed, and the caller's trace is overwritten by its coefficient arrays
};

// Ext words of dot-product scratch the openings of an AIR need (ext_dot_columns2 keeps two sets of partial sums of its widest matrix;
// the quotient has 8 columns)
inline size_t dot_scratch_words(const AirShape& s) { return 2 * (size_t)std::max({s.W1, s.Wp, 8u}) * div_up(s.H, 8192); }

inline streamed::Ctx stream_ctx(PwProver* p, const AirShape& s, const CommitLayout& L) {
    return streamed::Ctx{p, s.log_h, L.b, L.perm_panels, s.H, s.N, L.m, s.W, s.Wp};
}

// the constraint programs as the interpreter kernels take them (an AIR with public values: with the array of them)
inline ConstraintProgram constraint_program(const PwProver* p, uint32_t nc) {
    ConstraintProgram c{p->d_bytecode, p->d_spans, nc, p->is_xbc};
    if (p->n_public) { c.d_pub = p->d_pub; c.pub_base = p->pub_base; }
    return c;
}

inline LogupProgram logup_program(const PwProver* p, const AirShape& s) {
    return s.Wp ? LogupProgram{p->d_inter, s.n_int, p->d_ixspans, p->d_icode, p->d_gstarts, s.n_g, p->d_iforms} : LogupProgram{};
}

// ---- the buffer plan ---------------------------------------------------------------------------------------------------------
// Bytes of every device buffer of a prover object. The stage buffers (coef .. gbuf) are sized here for both provers; ext_arena and
// misc hold what the PROOF keeps beside the AIR's own vectors (FRI layers, openings, gamma powers, the query tail) and digests /
// tcoef / fscale exist only where one AIR carries its own trees or coefficient arrays: those are the caller's terms.
struct BufferPlan {
    size_t coef = 0, lde = 0, digests = 0, tcoef = 0, fscale = 0, perm = 0, plde = 0, q = 0, qpart = 0, qcoef = 0, qlde = 0, gbuf = 0,
           ext_arena = 0, misc = 0;
    size_t total() const { return coef + lde + digests + tcoef + fscale + perm + plde + q + qpart + qcoef + qlde + gbuf + ext_arena + misc; }
    // what the trace commitment alone needs (pw_prover_trace_root)
    BufferPlan commit_part() const { BufferPlan C; C.coef = coef; C.lde = lde; C.digests = digests; C.tcoef = tcoef; C.fscale = fscale; return C; }
};

// The stage buffers of one AIR in mode m, and the part of the layout that follows from them (H, N, b, m, panel_cols, perm_panels).
// eat: a streamed proof then keeps the trace's coefficient arrays IN the caller's buffer; with LogUp the permutation matrix is computed
// into `lde` first (its evaluations are only needed until its coefficients exist), while `perm` lends its room to the trace's
// coefficients until the trace itself is dead.
inline void plan_stage_buffers(const PwProver* p, const AirShape& s, AirMode m, CommitLayout& L, BufferPlan& B) {
    const size_t H = s.H, N = s.N;
    const bool lg = s.Wp != 0;
    const int b = m.b;
    L.H = H; L.N = N; L.b = b; L.m = N >> b;
    // coefficients exist only per column panel (1 GB by default; larger panels = fewer, larger launches): iNTT -> panel ->
    // coset NTT into the resident LDE. Streamed: the panel serves the eight phi / row-sum columns only.
    L.panel_cols = lde_panel_cols(H, b ? 8 : std::max<size_t>(s.W, s.Wp));
    B.coef = L.panel_cols * H * 4;
    // streamed: `lde` holds one sub-coset. The commitments and the query rows take the two matrices one after the other (max(W, Wp)
    // columns); the quotient needs main AND permutation columns of the same rows — all of them for the interpreter, but a unit of the
    // specialised LogUp kernels reads only the columns of its own groups: the main block + one unit's panel. That is what lets
    // configs[2] run with 4 sub-cosets instead of 8 (half the coefficient re-reads, the transforms' first stage group is bound by them).
    L.perm_panels = b && lg && specialised(p) && !getenv("POWDR_STREAM_NO_PANELS");
    // resident: the fixed matrix's LDE rides behind the main columns, the row layout's values behind both
    if (!b) B.lde = ((size_t)s.W1 + s.Wr) * N * 4;
    else if (L.perm_panels) B.lde = std::max<size_t>(std::max(s.W, s.Wp), (size_t)s.W + quotient_max_unit_perm_cols(p)) * L.m * 4;
    else B.lde = (size_t)(s.W + s.Wp) * L.m * 4;
    if (b || s.log_h >= kDeepComboMinLogHeight) B.gbuf = (size_t)24 * H * 4;  // the DEEP combinations and their LDE
    if (lg) {  // + the uncommitted per-row-sum columns (kJitExtraPermCols; the streamed path keeps them on every path)
        B.perm = (size_t)(s.Wp + kJitExtraPermCols) * H * 4;
        B.plde = b ? (size_t)8 * N * 4 : (size_t)(s.Wp + kJitExtraPermCols) * N * 4;
    }
    B.q = 4 * N * 4;
    const size_t q_rows = L.m;
    if (!lg) {
        const uint32_t chunks = quotient_chunks(q_rows, s.nc);
        if (chunks > 1) B.qpart = (size_t)chunks * 4 * q_rows * 4;
    }
    if (b) B.qpart += 4 * L.m * 4;  // the interpreter kernels' unscaled sums of one sub-coset
    // the specialised kernels' partial sums (0 when there are none; ADVICE r3: not lazily in the middle of the proof, while other
    // AIRs' side streams run)
    B.qpart = std::max(B.qpart, jit_part_bytes(p, H, q_rows));
    if (b && m.eat && lg) {
        B.perm = std::max(B.perm, (size_t)s.W * H * 4);
        B.lde = std::max(B.lde, (size_t)(s.Wp + kJitExtraPermCols) * H * 4);
    }
    B.qcoef = 8 * H * 4;
    B.qlde = 8 * N * 4;
}

// Every device buffer of a prover object, listed ONCE: the planned ones with their entry of the plan, then those made outside a
// proof's plan (preprocessed columns, the mock provers' row values and bus order). apply_plan, pw_prover_destroy and
// pw_prover_device_bytes all walk these two tables.
constexpr struct { DeviceBuf PwProver::*buf; size_t BufferPlan::*bytes; } kPlannedBuffers[] = {
    {&PwProver::coef, &BufferPlan::coef}, {&PwProver::lde, &BufferPlan::lde}, {&PwProver::digests, &BufferPlan::digests},
    {&PwProver::tcoef, &BufferPlan::tcoef}, {&PwProver::fscale, &BufferPlan::fscale}, {&PwProver::perm, &BufferPlan::perm},
    {&PwProver::plde, &BufferPlan::plde}, {&PwProver::q, &BufferPlan::q}, {&PwProver::qpart, &BufferPlan::qpart},
    {&PwProver::qcoef, &BufferPlan::qcoef}, {&PwProver::qlde, &BufferPlan::qlde}, {&PwProver::ext_arena, &BufferPlan::ext_arena},
    {&PwProver::misc, &BufferPlan::misc}, {&PwProver::gbuf, &BufferPlan::gbuf}};
constexpr DeviceBuf PwProver::*kUnplannedBuffers[] = {&PwProver::pre_vals, &PwProver::pre_lde, &PwProver::pre_tree, &PwProver::row_vals,
                                                      &PwProver::bus_order};
template <class P, class F>
inline void for_each_buffer(P* p, F&& f) {
    for (const auto& e : kPlannedBuffers) f(p->*e.buf);
    for (const auto m : kUnplannedBuffers) f(p->*m);
}

// grows the prover's buffers to a plan (nothing shrinks; a zero entry is a buffer the plan does not use)
inline int apply_plan(PwProver* p, const BufferPlan& B) {
    for (const auto& e : kPlannedBuffers)
        if (B.*e.bytes) PW_STRY((p->*e.buf).ensure(B.*e.bytes));
    return 0;
}

// ---- the proof sink ------------------------------------------------------------------------------------------------------------
// The proof's words and the transcript that sees them, together: what a proof writes is observed in the same call.
struct ProofSink {
    std::vector<uint32_t>& words;
    Challenger ch;
    explicit ProofSink(std::vector<uint32_t>& w) : words(w) { words.clear(); }
    void put(uint32_t canonical) { words.push_back(canonical); }  // written, not observed (the witness, a query index)
    void put_monty(const uint32_t* w, size_t n) { for (size_t i = 0; i < n; ++i) words.push_back(bb::from_monty(w[i])); }
    void put_raw(const uint32_t* w, size_t n) { words.insert(words.end(), w, w + n); }  // answers: canonical already
    void word(uint32_t x) { ch.observe_canonical(x % bb::P); put(x); }  // a header word
    void root(const uint32_t* r8) { put_monty(r8, 8); ch.observe_words(r8, 8); }  // a Merkle root (Montgomery)
    void ext(const bb::Ext& e) { put_monty(e.c, 4); ch.observe_ext(e); }
};

// ---- the stages --------------------------------------------------------------------------------------------------------------
// What the two provers place differently. Unused entries may be null (tcoef when resident, blpow / weights2 / rowsum without LogUp).
struct AirBufs {
    const uint32_t* trace;   // the caller's trace (W columns of H rows)
    const uint32_t* values;  // what the programs read on the trace domain: the trace, or with preprocessed columns the (trace | fixed) copy
    uint32_t* tcoef;         // streamed: the trace's coefficient arrays (eat: the caller's buffer itself)
    bb::Ext* apow;           // alpha^(M - 1) .. alpha^0
    bb::Ext* blpow;          // beta^0 .. beta^(max_args + 1)
    bb::Ext* weights;        // H: the weights at zeta
    bb::Ext* weights2;       // H: the weights at g zeta
    bb::Ext* rowsum;         // H + H / 4096 + 1: LogUp per-row sums, then block totals
    bb::Ext* scratch;        // dot_scratch_words
};

// From the trace values to the permutation matrix's LDE in p->plde (resident), or to its coefficient arrays in p->perm plus the eight
// extended phi / row-sum columns in p->plde (streamed). s_words[k]: the device address of coordinate k of S = phi(last row), valid
// until the next stage of this prover that uses p->gbuf. Committing the matrix and fetching S are the caller's.
inline int logup_stage(PwProver* p, const AirShape& s, AirMode m, const CommitLayout& L, const AirBufs& B, bb::Ext al, const uint32_t* s_words[4]) {
    const size_t H = s.H;
    const bool jit = specialised(p);
    uint32_t* d_perm = p->perm.as<uint32_t>();
    // eat: the matrix's VALUES live in the sub-coset buffer (idle between two passes) until its coefficient arrays exist
    uint32_t* d_pval = m.eat ? p->lde.as<uint32_t>() : d_perm;
    if (jit) PW_STRY(logup_perm_trace_jit(p, B.values, H, al, B.blpow, d_pval, B.rowsum, B.rowsum + H));
    else PW_STRY(logup_perm_trace(B.values, H, logup_program(p, s), al, B.blpow, d_pval, B.rowsum, B.rowsum + H));
    const uint32_t* phi_last = d_pval + ((size_t)(4 * s.n_g) * H + (H - 1));
    if (!m.b) {
        PW_STRY(lde_matrix(p, L, s.log_h, d_perm, s.Wp + (jit ? kJitExtraPermCols : 0u), p->plde.as<uint32_t>()));
        for (int k = 0; k < 4; ++k) s_words[k] = phi_last + (size_t)k * H;
        return 0;
    }
    // streamed: only phi and the per-row sums (the boundary terms read them at rows j and j + 2) are extended for good
    if (!jit) PW_STRY(ext_to_cols(B.rowsum, H, d_pval + (size_t)(4 * s.n_g + 4) * H));
    PW_STRY(lde_matrix(p, L, s.log_h, d_pval + (size_t)(4 * s.n_g) * H, 8, p->plde.as<uint32_t>()));
    // S is parked before the matrix becomes its coefficient arrays in place (device to device: no host round trip inside a stage)
    uint32_t* d_save = p->gbuf.as<uint32_t>();
    for (int k = 0; k < 4; ++k) {
        PW_HIP_TRY(hipMemcpyAsync(d_save + k, phi_last + (size_t)k * H, 4, hipMemcpyDeviceToDevice, stream()));
        s_words[k] = d_save + k;
    }
    if (m.eat) {
        // the trace's values are dead now: its coefficient arrays (waiting in p->perm) move into its place, the permutation buffer
        // takes the matrix's
        PW_HIP_TRY(hipMemcpyAsync(B.tcoef, d_perm, (size_t)s.W * H * 4, hipMemcpyDeviceToDevice, stream()));
        PW_STRY(intt_dif(d_pval, d_perm, H, H, s.Wp, (int)s.log_h));
    } else PW_STRY(intt_dif(d_perm, d_perm, H, H, s.Wp, (int)s.log_h));
    return 0;
}

// Z_H(x) = x^H - 1 on the even / odd rows of the shifted domain of 2H points: x_j^H = s^H (-1)^j
inline void vanishing_on_coset(uint32_t log_h, uint32_t* zv_even, uint32_t* zv_odd) {
    const uint32_t one = bb::R_MOD_P;
    uint32_t sH = bb::to_monty(field::kCosetShift);
    for (uint32_t i = 0; i < log_h; ++i) sH = bb::sqr(sH);
    *zv_even = bb::sub(sH, one);
    *zv_odd = bb::sub(bb::neg(sH), one);
}

// From the alpha powers to the quotient's chunk coefficients in p->qcoef and their LDE in p->qlde (p->q: the quotient over N rows)
inline int quotient_stage(PwProver* p, const AirShape& s, AirMode m, const CommitLayout& L, const AirBufs& B, bb::Ext al, bb::Ext S) {
    const bool lg = s.Wp != 0, jit = specialised(p);
    uint32_t zv_even, zv_odd;
    vanishing_on_coset(s.log_h, &zv_even, &zv_odd);
    const ConstraintProgram prog = constraint_program(p, s.nc);
    uint32_t* d_lde = p->lde.as<uint32_t>();
    uint32_t* d_plde = p->plde.as<uint32_t>();
    uint32_t* d_q = p->q.as<uint32_t>();
    if (m.b) {
        // streamed: the terms that read the current row only, sub-coset by sub-coset (unscaled sums scattered to their rows of d_q), then
        // the boundary terms / the division by Z_H over all rows
        PW_STRY(streamed::quotient_sums(stream_ctx(p, s, L), jit, lg, s.nc, prog, logup_program(p, s), B.tcoef, p->perm.as<uint32_t>(), B.apow, al,
                                        B.blpow, S, s.logN, d_q));
        if (lg) PW_STRY(quotient_logup_tail(d_q, 1, d_plde, d_plde + 4 * s.N, s.N, s.logN, B.apow + s.nc + s.n_g, S, zv_even, zv_odd, d_q));
        else PW_STRY(quotient_combine(d_q, 1, s.N, bb::inv(zv_even), bb::inv(zv_odd), d_q));
    } else if (lg && jit)
        PW_STRY(quotient_eval_logup_jit(p, d_lde, d_plde, s.N, s.logN, B.apow, al, B.blpow, S, zv_even, zv_odd, d_q));
    else if (lg)
        PW_STRY(quotient_eval_logup(d_lde, d_plde, s.N, s.logN, prog, logup_program(p, s), B.apow, al, B.blpow, S, zv_even, zv_odd, d_q));
    else if (jit && s.nc)
        PW_STRY(quotient_eval_jit(p, d_lde, s.N, B.apow, bb::inv(zv_even), bb::inv(zv_odd), d_q));
    else
        PW_STRY(quotient_eval(d_lde, s.N, prog, B.apow, bb::inv(zv_even), bb::inv(zv_odd), d_q, p->qpart.as<uint32_t>(), quotient_chunks(s.N, s.nc)));
    PW_STRY(intt_dif(d_q, d_q, s.N, s.N, 4, s.logN));
    PW_STRY(quotient_split(d_q, s.H, (int)s.log_h, p->qcoef.as<uint32_t>()));
    return coset_lde_from_coeffs(p->qcoef.as<uint32_t>(), p->qlde.as<uint32_t>(), s.H, s.N, 8, (int)s.log_h);
}

// All openings of one AIR into o[0 .. K): main | preprocessed | perm at zeta | quotient | perm at g zeta [| main | preprocessed at g zeta].
// Trace columns: barycentric evaluation straight from the values on the trace domain (a two-point AIR: at zeta and at g zeta in one
// pass); a trace that is its coefficient arrays by now (eat), a streamed permutation matrix and the quotient chunks: zeta weights on
// the coefficients. The permutation matrix is opened in the column slices [slice_at[i], slice_at[i + 1]), i < n_slices (at zeta and at
// g zeta in one pass over a slice); after_piece() runs when a piece has been enqueued — the main columns, each slice, the quotient —
// so that a caller may mark the stream there and consume the pieces one by one.
template <class AfterPiece>
inline int open_stage(PwProver* p, const AirShape& s, AirMode m, const AirBufs& B, bb::Ext zeta, bb::Ext gzeta, bb::Ext* o, const uint32_t* slice_at,
                      uint32_t n_slices, AfterPiece&& after_piece) {
    const int log_h = (int)s.log_h;
    const size_t H = s.H;
    auto open_perm = [&]() -> int {
        for (uint32_t i = 0; i < n_slices; ++i) {
            const uint32_t c0 = slice_at[i], c1 = slice_at[i + 1];
            if (c1 > c0)
                PW_STRY(ext_dot_columns2(p->perm.as<uint32_t>() + (size_t)c0 * H, H, c1 - c0, H, B.weights, B.weights2, o + s.W1 + c0, o + s.K1 + c0, B.scratch));
            PW_STRY(after_piece());
        }
        return 0;
    };
    if (!m.eat) {
        PW_STRY(barycentric_weights(zeta, log_h, B.weights));
        if (s.Wg) {
            PW_STRY(barycentric_weights(gzeta, log_h, B.weights2));
            PW_STRY(ext_dot_columns2(B.values, H, s.W1, H, B.weights, B.weights2, o, o + s.K1 + s.Wp, B.scratch));
        } else
            PW_STRY(ext_dot_columns(B.values, H, s.W1, H, B.weights, o, B.scratch));
        PW_STRY(after_piece());
    }
    if (s.Wp && !m.b) {
        if (!s.Wg) PW_STRY(barycentric_weights(gzeta, log_h, B.weights2));
        PW_STRY(open_perm());
    }
    PW_STRY(zeta_weights(zeta, log_h, B.weights));
    if (m.eat) {  // the trace is its coefficient arrays by now: opened like the permutation matrix below
        PW_STRY(ext_dot_columns(B.tcoef, H, s.W, H, B.weights, o, B.scratch));
        PW_STRY(after_piece());
    }
    if (s.Wp && m.b) {  // streamed: p->perm holds the matrix's coefficient arrays
        PW_STRY(zeta_weights(gzeta, log_h, B.weights2));
        PW_STRY(open_perm());
    }
    PW_STRY(ext_dot_columns(p->qcoef.as<uint32_t>(), H, 8, H, B.weights, o + s.W1 + s.Wp, B.scratch));
    return after_piece();
}

// The reduced-opening vector of one AIR into out (N Ext): v[j] = (sum_k gamma^k P_k(x_j) - sum1) / (x_j - zeta) + the same over the
// polynomials opened at g zeta with sum2. d_gpow: the AIR's K centred gamma powers in the order of open_stage. sums() fills sum1 and
// sum2 on the host; it is called AFTER the first launches of the arm taken, so that the device works meanwhile (the DEEP numerator is
// a polynomial: from 2^kDeepComboMinLogHeight rows on it is combined on the un-extended matrices — half the bytes their LDE holds —
// and extended as 4 + 4 columns, two launches that hide the sums; shorter traces keep the one-kernel form over the LDE).
template <class Sums>
inline int deep_stage(PwProver* p, const AirShape& s, AirMode m, const CommitLayout& L, const AirBufs& B, const bb::Ext* d_gpow, bb::Ext gamma,
                      Sums&& sums, const bb::Ext& sum1, const bb::Ext& sum2, bb::Ext zeta, bb::Ext gzeta, bb::Ext* out) {
    const bool lg = s.Wp != 0;
    uint32_t* d_lde = p->lde.as<uint32_t>();
    uint32_t* d_plde = p->plde.as<uint32_t>();
    uint32_t* d_qlde = p->qlde.as<uint32_t>();
    if (m.b)  // streamed: combined on the coefficient arrays (one pass over them); the eight quotient columns join from their resident LDE
        return streamed::deep_from_coefficients(stream_ctx(p, s, L), lg, B.tcoef, p->perm.as<uint32_t>(), d_qlde, s.logN, d_gpow, sums, sum1, sum2, zeta,
                                                gzeta, out);
    if (s.Wg) {  // two-point: the W1 columns at both points from one read of their LDE
        sums();
        return deep_quotient_two_point(d_lde, s.W1, lg ? d_plde : nullptr, s.Wp, d_qlde, s.N, s.logN, d_gpow, bb::ext_pow(gamma, s.K1 + s.Wp), sum1, sum2,
                                       zeta, gzeta, out);
    }
    if (s.log_h >= kDeepComboMinLogHeight && !s.Wf && !getenv("POWDR_DEEP_DIRECT") && !((uintptr_t)B.trace & 7)) {  // (the combination reads 8-byte pairs)
        // resident and tall: the same combination on the evaluations over <g_n> (the caller's trace, the permutation matrix), extended
        // like any column
        uint32_t* d_gev = p->gbuf.as<uint32_t>();
        uint32_t* d_glde = d_gev + 8 * s.H;
        PW_STRY(ext_lincomb(B.trace, s.W, p->perm.as<uint32_t>(), s.Wp, s.H, d_gpow, lg ? s.K1 : 0u, d_gev));
        PW_STRY(lde_matrix(p, L, s.log_h, d_gev, lg ? 8u : 4u, d_glde));
        sums();  // (the device is busy with the two launches above)
        return deep_from_combo(d_glde, d_qlde, s.N, s.logN, d_gpow + s.W + s.Wp, sum1, sum2, zeta, gzeta, lg ? 1 : 0, out);
    }
    sums();
    if (lg) return deep_quotient_logup(d_lde, s.W1, d_plde, s.Wp, d_qlde, s.N, s.logN, d_gpow, sum1, sum2, zeta, gzeta, out);
    return deep_quotient(d_lde, s.W1, d_qlde, 8, s.N, s.logN, d_gpow, sum1, zeta, out);
}

// One FRI commit round: the tree over the pairs (v[i], v[i + half]) into `digests`, its root (Montgomery) to the host. Synchronises:
// the next fold needs the challenge drawn from the root.
inline int fri_commit_round(const bb::Ext* v, size_t half, uint32_t* digests, uint32_t* root8) {
    // the tree's tail kernel writes the root into host-mapped memory: no copy dispatch between the layers
    uint32_t* d_mail = nullptr;
    uint32_t* h_mail = merkle_root_mailbox(&d_mail);
    PW_STRY(merkle_commit_ext_pairs(v, half, digests, h_mail ? d_mail : nullptr));
    if (!h_mail) PW_HIP_TRY(hipMemcpyAsync(root8, digests + merkle_words(half) - 8, 32, hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    if (h_mail) memcpy(root8, h_mail, 32);
    return 0;
}

// The proof-of-work search on a transcript's parts: the sponge state and the in_len <= 7 observed words not yet absorbed (Montgomery
// words); *witness = the smallest one. d_scratch: 25 words.
inline int grind_search(const uint32_t* st16, const uint32_t* in, size_t in_len, uint32_t pow_bits, uint32_t* d_scratch, uint32_t* witness) {
    uint32_t pending[8] = {0};
    for (size_t i = 0; i < in_len; ++i) pending[i] = in[i];
    PW_HIP_TRY(hipMemcpyAsync(d_scratch, st16, 64, hipMemcpyHostToDevice, stream()));
    PW_HIP_TRY(hipMemcpyAsync(d_scratch + 16, pending, 32, hipMemcpyHostToDevice, stream()));
    return pow_grind(d_scratch, d_scratch + 16, (uint32_t)in_len, pow_bits, d_scratch + 24, witness);
}

// Proof of work on the transcript as it stands: *witness (0 when pow_bits is 0) is observed and the bits are drawn. d_scratch: 25 words.
inline int grind(Challenger& ch, uint32_t pow_bits, uint32_t* d_scratch, uint32_t* witness) {
    *witness = 0;
    if (pow_bits) PW_STRY(grind_search(ch.st, ch.in.data(), ch.in.size(), pow_bits, d_scratch, witness));
    ch.observe_canonical(*witness);
    if (pow_bits) (void)ch.sample_bits((int)pow_bits);
    return 0;
}

// The FRI layers of a domain of 2^logN points: layer l (N >> l Ext) at layer_off[l], l <= logN - 1, and its tree at tree_off[l] words
struct FriLayout {
    std::vector<size_t> layer_off, tree_off;
    size_t fri_words = 0;  // all trees together
    explicit FriLayout(int logN) : layer_off(logN), tree_off(logN - 1) {
        const size_t N = (size_t)1 << logN;
        size_t o = 0;
        for (int l = 0; l < logN; ++l) { layer_off[l] = o; o += N >> l; }
        for (int l = 0; l + 1 < logN; ++l) { tree_off[l] = fri_words; fri_words += merkle_words((N >> l) / 2); }
    }
};

// The FRI part of the answer to query index q: per layer the sibling's offset in the layer arena (in words) and the offsets of the
// path's sibling digests in the digest arena, whose FRI trees start at word fri_base
inline void fri_query_offsets(size_t q, int logN, const FriLayout& F, size_t fri_base, std::vector<uint64_t>& ext_offs, std::vector<uint64_t>& dig_offs) {
    const size_t N = (size_t)1 << logN;
    for (int l = 0; l < logN - 1; ++l) {
        const size_t Nl = N >> l, half = Nl / 2, pp = q & (Nl - 1);
        ext_offs.push_back((F.layer_off[l] + (pp ^ half)) * 4);
        const size_t leaf = pp & (half - 1);
        for (int lv = 0; lv < logN - 1 - l; ++lv)
            dig_offs.push_back(fri_base + F.tree_off[l] + merkle_level_offset(half, lv) + (((leaf >> lv) ^ 1) * 8));
    }
}

// The FRI commit phase over the layers at d_v (F's offsets), trees into d_fdig: per round the tree of the layer, its root into the
// proof, the challenge, the fold — with `shift` squared from round to round (R_MOD_P: the unshifted subgroups, which stay so) —
// and roll_in(l, beta, next layer, its length) for what the caller adds to the folded layer; then the final polynomial.
template <class RollIn>
inline int fri_commit_phase(ProofSink& pf, const FriLayout& F, int logN, bb::Ext* d_v, uint32_t* d_fdig, uint32_t shift, RollIn&& roll_in) {
    const size_t N = (size_t)1 << logN;
    uint32_t root[8];
    for (int l = 0; l + 1 < logN; ++l) {
        const size_t half = (N >> l) / 2;
        bb::Ext* v = d_v + F.layer_off[l];
        bb::Ext* nv = d_v + F.layer_off[l + 1];
        PW_STRY(fri_commit_round(v, half, d_fdig + F.tree_off[l], root));
        pf.root(root);
        const bb::Ext beta = pf.ch.sample_ext();
        PW_STRY(fri_fold(v, half, logN - l, shift, beta, nv));
        PW_STRY(roll_in(l, beta, nv, half));
        shift = bb::sqr(shift);
    }
    bb::Ext final_poly;
    PW_HIP_TRY(hipMemcpyAsync(&final_poly, d_v + F.layer_off[logN - 1], sizeof(bb::Ext), hipMemcpyDeviceToHost, stream()));
    PW_HIP_TRY(hipStreamSynchronize(stream()));
    pf.ext(final_poly);
    return 0;
}
inline int no_roll_in(int, const bb::Ext&, bb::Ext*, size_t) { return 0; }

// The query answers that are digests and FRI siblings, to the host as canonical words: the offsets go up to d_offs (digest offsets,
// then ext offsets), the records are gathered from the digest arena and the layer arena into d_dig_out / d_ext_out; more_digests()
// may gather n_more further digest records behind those; ONE synchronisation, which also ends whatever the caller enqueued before.
template <class MoreDigests>
inline int fetch_query_answers(const uint32_t* d_dig, const bb::Ext* d_v, const std::vector<uint64_t>& dig_offs, const std::vector<uint64_t>& ext_offs,
                               uint64_t* d_offs, uint32_t* d_dig_out, uint32_t* d_ext_out, size_t n_more, MoreDigests&& more_digests,
                               std::vector<uint32_t>& dig, std::vector<uint32_t>& ext) {
    const size_t nd = dig_offs.size(), ne = ext_offs.size();
    const hipStream_t st = stream();
    PW_HIP_TRY(hipMemcpyAsync(d_offs, dig_offs.data(), nd * 8, hipMemcpyHostToDevice, st));
    if (ne) PW_HIP_TRY(hipMemcpyAsync(d_offs + nd, ext_offs.data(), ne * 8, hipMemcpyHostToDevice, st));
    PW_STRY(gather_records(d_dig, d_offs, 8u, (uint32_t)nd, d_dig_out));
    PW_STRY(gather_records(reinterpret_cast<const uint32_t*>(d_v), d_offs + nd, 4u, (uint32_t)ne, d_ext_out));
    PW_STRY(more_digests());
    PW_STRY(canonicalize_words(d_dig_out, (nd + n_more) * 8));
    PW_STRY(canonicalize_words(d_ext_out, ne * 4));
    dig.resize((nd + n_more) * 8 + 1);
    ext.resize(ne * 4 + 1);
    PW_HIP_TRY(hipMemcpyAsync(dig.data(), d_dig_out, (nd + n_more) * 32, hipMemcpyDeviceToHost, st));
    if (ne) PW_HIP_TRY(hipMemcpyAsync(ext.data(), d_ext_out, ne * 16, hipMemcpyDeviceToHost, st));
    PW_HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the FRI part of one query's answer (fri_query_offsets' order): per round the sibling value, then the path's digests
inline void put_fri_answer(ProofSink& pf, int logN, const std::vector<uint32_t>& dig, const std::vector<uint32_t>& ext, size_t& dpos, size_t& epos) {
    for (int l = 0; l + 1 < logN; ++l) {
        pf.put_raw(&ext[epos * 4], 4);
        epos += 1;
        const size_t depth = (size_t)logN - 1 - l;
        pf.put_raw(&dig[dpos * 8], depth * 8);
        dpos += depth;
    }
}

#undef PW_STRY

}  // namespace pw
