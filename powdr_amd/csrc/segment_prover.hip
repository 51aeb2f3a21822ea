// pw-stark v1 on the device: ONE proof for all AIRs of a segment (proof magic "PWS3").
//
// The reference makes one engine call per segment with the traces of all chips, `engine.prove(pk, ProvingContext{
// per_trace})` (/root/reference/openvm/src/trace_generation.rs:136-139, openvm-riscv/src/lib.rs:327-332). Protocol
// definition: oracle/stark_segment.inc (header comment); the words produced here must equal the oracle's.
//
// The per-AIR stages between the commitments (permutation matrix, quotient, openings, DEEP numerator, a FRI commit round, proof of
// work) are prover_stages.hpp's, shared with the one-AIR prover; this file keeps the protocol: trees, transcript, FRI fold, queries.
// prove_segment_impl at the end of the file is the protocol as a list; its phases, in order:
//   validate_airs, forced_modes_by_air   the arguments and the test hook's list: refused before anything is touched
//   (buffers)          the segment's own device arenas, every byte of them from SegLayout (segment_layout.hpp)
//   choose_modes       which AIRs are streamed: forced, or the memory policy (plan_segment_streams); then every AIR's buffers in its mode
//   write_header       header; preprocessed roots, row flags and public values into the transcript
//   commit_main        LDE of every main trace (lde_matrix, prover.hip), ONE mixed-height Poseidon2 tree over all of them
//                      (commit_mixed): the leaf hash runs over a column-pointer table, so all AIRs of one height are hashed by one
//                      launch — a 2^12-row AIR no longer gets a launch (and a quarter-empty GPU) of its own
//   commit_logup       LogUp permutation matrices (shared challenges straight from the segment transcript), one mixed tree
//   commit_quotient    quotients (shared alpha), one mixed tree over the 8-column chunk matrices
//   open_all           openings at zeta / g_a zeta, all AIRs' values fetched with one copy
//   reduce_openings    reduced openings per height
//   fri_commit_phase   (prover_stages.hpp) FRI over the tallest domain with the smaller heights rolled in; then grind
//   answer_queries     one query phase (gather_query_rows, fetch_query_answers)
// Host round trips per segment: 3 roots + 1 (sums) + 1 (openings) + L FRI roots + queries, instead of that per AIR.
//
// STREAMED AIRs (round 4): an AIR whose LDE does not fit beside the others — BASELINE configs[2]'s 3 731 + 4 632 committed
// columns x 2^23 rows — is proven from coefficient arrays inside the same segment proof: its row digests are hashed sub-coset by
// sub-coset into its level of the mixed trees (merkle.hip `external` levels), its quotient, DEEP numerator and query rows come from
// prover_stream.hpp. A level's row digest is a sponge over the CONCATENATED rows of all matrices of that height: a level that holds a
// streamed matrix is absorbed run by run with the rows' sponge states parked in between (merkle.hip leaf_absorb_kernel).
#include "prover_state.hpp"
#include "prover_stages.hpp"
#include "segment_layout.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pw;

#define TRY(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

namespace {

constexpr int kMaxSide = 8;
struct SegCtx {
    DeviceBuf dig;     // three mixed trees | FRI trees
    DeviceBuf inject;  // row digests of the smaller heights (one level at a time)
    DeviceBuf ext;     // FRI layers (2 N) | reduced openings of the smaller heights (N) | scratch vector (N)
    DeviceBuf misc;    // column-pointer tables, opened values, gamma powers, query indices / answers
    DeviceBuf state;   // streamed AIRs: the rows' sponge states of the level being hashed run by run (16 words per row)
    std::vector<uint32_t> proof;
    size_t last_plan[3] = {0, 0, 0};   // bytes of the last call's plan: all AIRs resident | as chosen | what the policy had to work with
    std::vector<uint32_t> last_modes;  // per AIR of the last call: log2(sub-cosets) | 0x100 if the trace was eaten (pw_segment_last_modes)
    // the byte tables the last call's memory policy planned with (pw::plan_segment_streams; tests: pw_segment_last_plan_tables)
    std::vector<size_t> plan_resident, plan_streamed;
    std::vector<int> plan_b_max;
    // the public values of the call's AIRs as they were set when it began: uploaded from here, so a caller that sets
    // new values after the call returns never races with a copy still in flight
    std::vector<std::vector<uint32_t>> pub_snapshot;
    // side streams for the per-AIR stages of a segment with many AIRs (fork from / join into the caller's stream by events)
    hipStream_t side[kMaxSide] = {};
    hipEvent_t fork_ev = nullptr, done_ev[kMaxSide] = {};
    int n_side = 0, side_device = -1;
    // device bytes the context holds now
    size_t bytes() const { return dig.bytes + inject.bytes + ext.bytes + misc.bytes + state.bytes; }
    int ensure_side(int want) {
        int dev = 0;
        PW_HIP_TRY(hipGetDevice(&dev));
        if (dev != side_device) { n_side = 0; fork_ev = nullptr; side_device = dev; }  // handles of another device are simply dropped
        if (!fork_ev) PW_HIP_TRY(hipEventCreateWithFlags(&fork_ev, hipEventDisableTiming));
        for (; n_side < want; ++n_side) {
            PW_HIP_TRY(hipStreamCreateWithFlags(&side[n_side], hipStreamNonBlocking));
            PW_HIP_TRY(hipEventCreateWithFlags(&done_ev[n_side], hipEventDisableTiming));
        }
        return 0;
    }
    // a host thread that proved segments exits: its streams, events and (through ~DeviceBuf) its device buffers go with it
    ~SegCtx() {
        int dev = -1;
        if (n_side == 0 && !fork_ev) return;
        if (hipGetDevice(&dev) != hipSuccess || dev != side_device) { (void)hipGetLastError(); return; }
        for (int k = 0; k < n_side; ++k) { (void)hipStreamDestroy(side[k]); (void)hipEventDestroy(done_ev[k]); }
        if (fork_ev) (void)hipEventDestroy(fork_ev);
    }
};
thread_local SegCtx g_ctx;  // one per host thread (= per launch stream)

// device buffers of one RESIDENT AIR in the segment flow (the per-AIR prover object owns them; nothing here is freed per segment):
// the sizes first — the streaming decision below adds up exactly what ensure_air would allocate — then the allocation.
// To the stage buffers the AIR adds only its own vectors: trees, FRI layers, openings, gamma powers and the query tail are the segment's.
BufferPlan plan_air(const PwProver* p, const AirShape& s, CommitLayout& Lc) {
    BufferPlan B;
    plan_stage_buffers(p, s, AirMode{0, false}, Lc, B);
    Lc.tree_words = 0; Lc.fri_words = 0; Lc.n_trees = 0;
    B.ext_arena = (3 * s.H + s.H / 4096 + 32) * sizeof(bb::Ext);  // weights | weights at g zeta | row sums + block totals
    B.misc = (dot_scratch_words(s) + s.M + p->max_args + 64) * sizeof(bb::Ext) + 4096;  // scratch | alpha, beta powers
    return B;
}
int ensure_air(PwProver* p, const AirShape& s, CommitLayout& Lc) { return apply_plan(p, plan_air(p, s, Lc)); }

}  // namespace

namespace pw {
// The streaming plan of a segment under a device budget, as a pure function of byte tables (CPU tests: pw_segment_stream_plan).
// resident[a]: AIR a with its LDE resident; streamed[a * 5 + b - 1]: streamed over 2^b sub-cosets (incl. its level's parked sponge
// states); b_max[a]: 0 = may not be streamed, else the most log2(sub-cosets) it may take. Round by round: first the largest AIRs with
// TWO sub-cosets each until the segment fits; only when every AIR that may be streamed is, four sub-cosets (largest first again), and
// so on. (Round 5's order — one AIR taken to 32 sub-cosets before the next is touched — cost a C4 segment under a 0.8 budget 905 ms
// instead of 452: a sub-coset pass has a fixed cost per column, and 2 sub-cosets of three AIRs re-read far less than 32 of one.
// profiles/r06_c4_budget_sweep.txt.) Equal sizes keep index order. sbv[a] := log2(sub-cosets) (0 = resident); returns the bytes
// planned, own + what every AIR needs in its mode: more than avail when nothing more helps.
size_t plan_segment_streams(size_t A, const size_t* resident, const size_t* streamed, const int* b_max, size_t own, size_t avail, int* sbv) {
    std::vector<size_t> bytes(resident, resident + A), order(A);
    size_t need = own;
    for (size_t a = 0; a < A; ++a) { need += bytes[a]; sbv[a] = 0; order[a] = a; }
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return bytes[x] > bytes[y]; });
    for (int b = 1; b <= 5 && need > avail; ++b) {
        for (size_t k = 0; k < A && need > avail; ++k) {
            const size_t a = order[k];
            if (b > b_max[a]) continue;
            const size_t nb = streamed[a * 5 + (b - 1)];
            if (nb >= bytes[a]) continue;
            need = need - bytes[a] + nb;
            bytes[a] = nb;
            sbv[a] = b;
        }
    }
    return need;
}
}  // namespace pw


namespace {

// The per-AIR stages (LDE, permutation trace, quotient, openings, query rows) of different AIRs are independent chains of
// small launches; on one stream a segment of 60 AIRs pays ~10 us of dispatch latency between 1 400 dependent kernels
// (profiles/r02_segment_gaps.txt: 15 of 176 ms). With K side streams the chains of different AIRs overlap:
// fork = the side streams wait for what the caller's stream has done, AIR a runs on side[a % K], join = the caller's stream
// waits for all of them. POWDR_SEGMENT_STREAMS=0 keeps everything on the caller's stream. Whatever way the call ends, the
// caller's stream is the current one again.
struct Fan {
    SegCtx& cx;
    hipStream_t st;
    int K = 0;
    ~Fan() { set_stream(st); }
    int open(size_t A) {
        const char* e = getenv("POWDR_SEGMENT_STREAMS");
        const int k = std::min(e ? atoi(e) : 4, kMaxSide);
        if (k < 2 || A < 4) return 0;
        TRY(cx.ensure_side(k));
        K = k;
        return 0;
    }
    int fork() {
        if (!K) return 0;
        PW_HIP_TRY(hipEventRecord(cx.fork_ev, st));
        for (int k = 0; k < K; ++k) PW_HIP_TRY(hipStreamWaitEvent(cx.side[k], cx.fork_ev, 0));
        return 0;
    }
    void on_air(size_t a) { if (K) set_stream(cx.side[a % (size_t)K]); }
    int join() {
        if (!K) return 0;
        set_stream(st);
        for (int k = 0; k < K; ++k) {
            PW_HIP_TRY(hipEventRecord(cx.done_ev[k], cx.side[k]));
            PW_HIP_TRY(hipStreamWaitEvent(st, cx.done_ev[k], 0));
        }
        return 0;
    }
    // per_air(a) for every AIR, each on its side stream, between a fork and a join
    template <class PerAir>
    int each(size_t A, PerAir&& per_air) {
        TRY(fork());
        for (size_t a = 0; a < A; ++a) { on_air(a); TRY(per_air(a)); }
        return join();
    }
};

// What the phases of one call share.
struct Seg {
    const PwSegmentAir* airs;
    const size_t A;
    const bool lg;
    const PwStarkConfig cfg;
    SegCtx& cx;
    hipStream_t st;  // the caller's (launch) stream
    Fan fan;
    ProofSink pf;
    std::vector<AirShape> sh;
    SegLayout y;
    // handed[a]: the caller gives the trace away (the reference moves `common_main` into the engine for EVERY AIR of a segment,
    // cuda/mod.rs:415-419). Only a STREAMED AIR uses that (eat[a]): its coefficient arrays then live in the caller's buffer.
    std::vector<char> handed, eat;
    std::vector<int> sbv;  // log2 of the number of sub-cosets, 0 = LDE resident
    std::vector<CommitLayout> Lc;
    MiscArena m{};
    uint32_t* d_dig = nullptr;   // the mixed trees | the FRI trees
    bb::Ext* d_v = nullptr;      // the ext arena
    std::vector<const uint32_t*> h_cols;  // commit_mixed's column table on its way to the device

    Seg(const PwSegmentAir* airs_, size_t A_, bool lg_, std::vector<char> handed_, SegCtx& c, hipStream_t s)
        : airs(airs_), A(A_), lg(lg_), cfg(airs_[0].prover->cfg), cx(c), st(s), fan{c, s}, pf(c.proof), sh(A_), handed(std::move(handed_)),
          eat(A_, 0), sbv(A_, 0), Lc(A_) {
        for (size_t a = 0; a < A; ++a) sh[a] = air_shape(airs[a].prover, airs[a].log_height, lg);
        y = SegLayout(sh, cfg.num_queries, lg);
    }
    PwProver* prover(size_t a) const { return airs[a].prover; }
    streamed::Ctx sctx(size_t a) const { return stream_ctx(prover(a), sh[a], Lc[a]); }
    AirMode mode_of(size_t a) const { return AirMode{sbv[a], eat[a] != 0}; }
    // A streamed AIR's trace coefficients: in its prover's tcoef — or, handed over (eat), in the caller's own buffer from the moment
    // nothing reads the trace's VALUES any more. With LogUp the permutation columns are computed from the values after the main
    // commitment, so the coefficients wait in the (still empty) permutation buffer until then (prover.hip prove_impl does the same).
    uint32_t* tcoef_of(size_t a) const { return eat[a] ? const_cast<uint32_t*>(airs[a].d_trace) : prover(a)->tcoef.as<uint32_t>(); }
    uint32_t* coef_first(size_t a) const { return eat[a] && lg ? prover(a)->perm.as<uint32_t>() : tcoef_of(a); }
    // the values the programs read on the trace domain: with preprocessed columns the prover's (trace | fixed matrix) copy
    const uint32_t* values_of(size_t a) const { return sh[a].Wf ? prover(a)->pre_vals.as<uint32_t>() : airs[a].d_trace; }
    // what the stages of AIR a read and write outside its prover's stage buffers: its vectors live in the prover's ext_arena
    // (weights | weights at g zeta | row sums + block totals) and misc (dot-product scratch | alpha powers | beta powers)
    AirBufs bufs_of(size_t a) const {
        bb::Ext* w = prover(a)->ext_arena.as<bb::Ext>();
        bb::Ext* scratch = prover(a)->misc.as<bb::Ext>();
        bb::Ext* apow = scratch + dot_scratch_words(sh[a]);
        return AirBufs{airs[a].d_trace, values_of(a), tcoef_of(a), apow, apow + sh[a].M + 4, w, w + sh[a].H, w + 2 * sh[a].H, scratch};
    }
};

// ---- validate ----------------------------------------------------------------------------------------------------------------
// honour_flags: pw_prove_segment_consuming — PwSegmentAir::flags is read (PW_AIR_HAND_OVER); pw_prove_segment ignores the word
// (callers of the older struct left it uninitialised)
int validate_airs(const PwSegmentAir* airs, size_t A, bool lg, bool honour_flags, std::vector<char>& handed) {
    handed.assign(A, 0);
    for (size_t a = 0; a < A; ++a) {
        handed[a] = honour_flags && (airs[a].flags & PW_AIR_HAND_OVER) ? 1 : 0;
        // a handed-over trace becomes a coefficient array that is read 2 / 4 words at a time (fold loads, the DEEP combination)
        if (handed[a] && ((uintptr_t)airs[a].d_trace & 15)) return (int)hipErrorInvalidValue;
        if (!airs[a].prover || !airs[a].d_trace || airs[a].log_height < 1 || airs[a].log_height > 26) return (int)hipErrorInvalidValue;
        if (lg && !airs[a].prover->logup) return (int)hipErrorInvalidValue;  // needs the interaction tables (pw_prover_create_logup)
        if (airs[a].prover->pre_width && airs[a].log_height != airs[a].prover->pre_log_h) return -1;  // the fixed matrix's height
        // one FRI / query phase means one configuration for all AIRs
        if (airs[a].prover->cfg.num_queries != airs[0].prover->cfg.num_queries || airs[a].prover->cfg.pow_bits != airs[0].prover->cfg.pow_bits)
            return (int)hipErrorInvalidValue;
        if (airs[a].prover->n_public && !airs[a].prover->pub_set) return -1;  // public values never set: not proven with zeros in their place
    }
    // the per-AIR device buffers live in the prover object and the AIRs of a segment run concurrently on side streams: one
    // prover cannot serve two AIRs of the same segment
    std::vector<const PwProver*> seen(A);
    for (size_t a = 0; a < A; ++a) seen[a] = airs[a].prover;
    std::sort(seen.begin(), seen.end());
    return std::adjacent_find(seen.begin(), seen.end()) != seen.end() ? (int)hipErrorInvalidValue : 0;
}

// ---- modes -------------------------------------------------------------------------------------------------------------------
// POWDR_STREAM_LOG_BLOCKS_BY_AIR=b0,b1,... (tests): the mode of every AIR of the call, 0 = resident, clamped to what the AIR may
// take (ignored for AIRs too short to stream); before POWDR_STREAM_LOG_BLOCKS. A list of another length is refused here, before
// any trace or buffer is touched.
int forced_modes_by_air(size_t A, std::vector<int>& by_air) {
    const char* e = getenv("POWDR_STREAM_LOG_BLOCKS_BY_AIR");
    if (!e) return 0;
    for (const char* c = e; *c;) {
        char* end = nullptr;
        const long v = strtol(c, &end, 10);
        if (end == c || v < 0 || (*end && *end != ',')) return (int)hipErrorInvalidValue;
        by_air.push_back((int)std::min<long>(v, 31));
        c = *end ? end + 1 : end;
    }
    return by_air.size() == A ? 0 : (int)hipErrorInvalidValue;
}

// Which AIRs are streamed (s.sbv, s.eat), and the record of the decision (last_plan, the plan tables, last_modes). Runs when the
// segment's own arenas exist: what they hold counts as `held` when the policy asks the device for room.
void choose_modes(Seg& s, const std::vector<int>& by_air) {
    SegCtx& cx = s.cx;
    const size_t A = s.A;
    cx.last_plan[0] = cx.last_plan[1] = cx.last_plan[2] = 0;
    cx.plan_resident.clear(); cx.plan_streamed.clear(); cx.plan_b_max.clear();
    // (AIRs that share a height: their level is hashed run by run); an AIR with preprocessed columns or the row layout is always resident
    // (and so is one with public values)
    auto may_stream = [&](size_t a) { return s.sh[a].log_h >= 3 && !s.sh[a].Wf && !s.sh[a].rf && !s.prover(a)->n_public; };
    auto b_max = [&](size_t a) { return std::min((int)s.sh[a].log_h - 1, 5); };
    size_t held = cx.bytes(), avail = 0;
    if (!by_air.empty()) {  // forced per AIR (tests: mixed levels)
        for (size_t a = 0; a < A; ++a) if (may_stream(a) && by_air[a] > 0) s.sbv[a] = std::min(by_air[a], b_max(a));
    } else if (const char* e = getenv("POWDR_STREAM_LOG_BLOCKS")) {  // forced (tests): every AIR that may be streamed is
        const int v = atoi(e);
        for (size_t a = 0; a < A && v > 0; ++a) if (may_stream(a)) s.sbv[a] = std::min(v, b_max(a));
    } else {
        for (size_t a = 0; a < A; ++a) held += pw_prover_device_bytes(s.prover(a));
        if (device_room(held, &avail)) {
            // what this call allocates: the segment's own arenas + per AIR exactly what ensure_air (resident) or ensure_proof_buffers
            // (streamed; a handed-over trace needs no tcoef) would (not the one-AIR plan, which counts trees and FRI layers
            // per AIR that a segment shares)
            const size_t own = s.y.own();
            cx.plan_resident.assign(A, 0); cx.plan_streamed.assign(A * 5, 0); cx.plan_b_max.assign(A, 0);
            size_t need = own;
            for (size_t a = 0; a < A; ++a) {
                cx.plan_resident[a] = plan_air(s.prover(a), s.sh[a], s.Lc[a]).total();
                need += cx.plan_resident[a];
                if (!may_stream(a) || s.sh[a].log_h < stream_min_log_height()) continue;
                cx.plan_b_max[a] = b_max(a);
                for (int b = 1; b <= cx.plan_b_max[a]; ++b)  // + the parked sponge states of its level (cx.state)
                    cx.plan_streamed[a * 5 + (b - 1)] =
                        proof_plan_bytes(s.prover(a), s.sh[a].log_h, b, s.handed[a] != 0) + (size_t)16 * 4 * ((size_t)1 << s.sh[a].logN);
            }
            cx.last_plan[0] = need;  // everything resident
            cx.last_plan[2] = avail;
            cx.last_plan[1] = plan_segment_streams(A, cx.plan_resident.data(), cx.plan_streamed.data(), cx.plan_b_max.data(), own, avail, s.sbv.data());
        }
    }
    cx.last_modes.assign(A, 0);
    for (size_t a = 0; a < A; ++a) {
        s.eat[a] = s.handed[a] && s.sbv[a] > 0;  // the trace is overwritten by its coefficient arrays
        cx.last_modes[a] = (uint32_t)s.sbv[a] | (s.eat[a] ? 0x100u : 0u);
    }
}

// ---- header and transcript -----------------------------------------------------------------------------------------------------
int write_header(Seg& s) {
    const size_t A = s.A;
    Challenger& ch = s.pf.ch;
    bool any_pre = false, any_rows = false, any_pub = false;
    for (size_t a = 0; a < A; ++a) { any_pre = any_pre || s.sh[a].Wf; any_rows = any_rows || s.sh[a].rf; any_pub = any_pub || s.prover(a)->n_public; }
    const uint32_t magic = any_pub ? kMagic6 : any_rows ? kMagic5 : any_pre ? kMagic4 : kMagic3;
    for (uint32_t x : {magic, (uint32_t)A, s.lg ? 1u : 0u, s.cfg.num_queries, s.cfg.pow_bits}) s.pf.word(x);
    for (size_t a = 0; a < A; ++a)
        for (uint32_t x : {s.sh[a].log_h, s.sh[a].W, s.sh[a].nc, s.sh[a].n_int}) s.pf.word(x);
    // the verifying key's preprocessed commitments: observed, not written
    for (size_t a = 0; a < A; ++a) {
        if (!s.sh[a].Wf) continue;
        ch.observe_canonical((uint32_t)a % bb::P);
        ch.observe_canonical(s.sh[a].Wf % bb::P);
        for (int k = 0; k < 8; ++k) ch.observe_canonical(s.prover(a)->pre_root[k]);
    }
    // which AIRs are row-aware, and how: derived from the programs, observed, not written
    for (size_t a = 0; a < A; ++a) {
        if (!s.sh[a].rf) continue;
        ch.observe_canonical((uint32_t)a % bb::P);
        ch.observe_canonical(s.sh[a].rf);
    }
    // the public values: written right after the header, observed here, and on their way to the device on the launch
    // stream — every kernel that reads them is enqueued behind this copy (the side streams fork from it)
    for (size_t a = 0; a < A; ++a) {
        const uint32_t np = s.prover(a)->n_public;
        if (!np) continue;
        const std::vector<uint32_t>& pv = s.cx.pub_snapshot[a];
        ch.observe_canonical((uint32_t)a % bb::P);
        ch.observe_canonical(np);
        ch.observe_words(pv.data(), np);
        s.pf.put_monty(pv.data(), np);
        PW_HIP_TRY(hipMemcpyAsync(s.prover(a)->d_pub, pv.data(), (size_t)np * 4, hipMemcpyHostToDevice, s.st));
    }
    return 0;
}

// ---- commitments ---------------------------------------------------------------------------------------------------------------
// Mixed commitment of one matrix per AIR into tree `tree` of the digest arena (main | quotient | perm): matrix_of(a, m, w) = (device
// pointer, width); heights are the AIRs' LDE heights. The root (Montgomery) is on its way to root_monty when this returns.
template <class MatrixOf>
int commit_mixed(Seg& s, MatrixOf&& matrix_of, int tree, uint32_t* root_monty) {
    SegCtx& cx = s.cx;
    const int L = s.y.L;
    std::vector<const uint32_t*>& h_cols = s.h_cols;
    h_cols.clear();
    uint32_t* dg = s.d_dig + (size_t)tree * s.y.tree_words;
    std::vector<MixedLevelCols> by_log(L + 1, MixedLevelCols{nullptr, 0});
    // a level that holds a streamed matrix is hashed RUN BY RUN (merkle.hip leaf_absorb_kernel): consecutive resident matrices
    // through their slice of the column-pointer table, a streamed matrix sub-coset by sub-coset, the rows' sponge states parked
    // in cx.state in between; the level is then `external` for merkle_commit_mixed (which only injects / compresses)
    struct Run { size_t first_col; uint32_t n_cols; size_t air; bool streamed; };
    std::vector<std::vector<Run>> runs(L + 1);
    for (int k = L; k >= 0; --k) {
        const size_t first = h_cols.size();
        bool any_streamed = false;
        for (size_t a = 0; a < s.A; ++a) any_streamed = any_streamed || (s.sh[a].logN == k && s.sbv[a] && tree != 1);
        for (size_t a = 0; a < s.A; ++a) {
            if (s.sh[a].logN != k) continue;
            const uint32_t* m; uint32_t w;
            matrix_of(a, m, w);  // a streamed AIR hands over the matrix's COEFFICIENT arrays (column stride H)
            if (s.sbv[a] && tree != 1) { runs[k].push_back(Run{0, w, a, true}); continue; }
            if (any_streamed) {
                if (runs[k].empty() || runs[k].back().streamed) runs[k].push_back(Run{h_cols.size(), 0, a, false});
                runs[k].back().n_cols += w;
            }
            for (uint32_t c = 0; c < w; ++c) h_cols.push_back(m + (size_t)c * s.sh[a].N);
        }
        by_log[k] = MixedLevelCols{s.m.cols + first, (uint32_t)(h_cols.size() - first)};
        by_log[k].external = any_streamed ? 1u : 0u;
    }
    PW_HIP_TRY(hipMemcpyAsync(s.m.cols, h_cols.data(), h_cols.size() * 8, hipMemcpyHostToDevice, s.st));
    for (int k = L; k >= 0; --k) {
        if (runs[k].empty()) continue;
        const size_t rows = (size_t)1 << k;
        TRY(cx.state.ensure(rows * 16 * 4));
        uint32_t* level_digests = k == L ? dg : cx.inject.as<uint32_t>() + rows * 8;
        uint32_t pos = 0;
        for (size_t i = 0; i < runs[k].size(); ++i) {
            const Run& r = runs[k][i];
            const bool first_run = i == 0, last_run = i + 1 == runs[k].size();
            if (!r.streamed) {
                TRY(merkle_leaf_absorb(nullptr, 0, s.m.cols + r.first_col, r.n_cols, pos, rows, 1, 0, cx.state.as<uint32_t>(), level_digests, first_run, last_run));
            } else {
                const uint32_t* coef; uint32_t w;
                matrix_of(r.air, coef, w);
                const streamed::Ctx c = s.sctx(r.air);
                TRY(streamed::for_each_subcoset(c, {streamed::CoefMatrix{coef, w}}, nullptr, [&](uint32_t sub) {
                    return merkle_leaf_absorb(c.p->lde.as<uint32_t>(), c.m, nullptr, w, pos, c.m, (size_t)1 << c.b, sub, cx.state.as<uint32_t>(), level_digests,
                                              first_run, last_run);
                }));
            }
            pos = (pos + r.n_cols) & 7u;
        }
    }
    TRY(merkle_commit_mixed(by_log.data(), L, dg, cx.inject.as<uint32_t>()));
    PW_HIP_TRY(hipMemcpyAsync(root_monty, dg + s.y.tree_words - 8, 32, hipMemcpyDeviceToHost, s.st));
    return 0;
}

// LDE of every main trace (a streamed AIR: its coefficient arrays), ONE mixed-height tree over all of them
int commit_main(Seg& s) {
    uint32_t root[8];
    TRY(s.fan.each(s.A, [&](size_t a) -> int {
        PwProver* p = s.prover(a);
        const AirShape& sh = s.sh[a];
        p->committed_trace = nullptr;
        // streamed: the trace's coefficient arrays; its LDE rows exist one sub-coset at a time from here on
        if (s.sbv[a]) return intt_dif(s.airs[a].d_trace, s.coef_first(a), sh.H, sh.H, sh.W, (int)sh.log_h);
        if (sh.Wf) {  // the trace in front of the fixed matrix, the fixed LDE behind the main columns (the tree hashes the first W)
            PW_HIP_TRY(hipMemcpyAsync(p->pre_vals.as<uint32_t>(), s.airs[a].d_trace, (size_t)sh.W * sh.H * 4, hipMemcpyDeviceToDevice, stream()));
            PW_HIP_TRY(hipMemcpyAsync(p->lde.as<uint32_t>() + (size_t)sh.W * sh.N, p->pre_lde.as<uint32_t>(), (size_t)sh.Wf * sh.N * 4,
                                      hipMemcpyDeviceToDevice, stream()));
        }
        TRY(lde_matrix(p, s.Lc[a], sh.log_h, s.airs[a].d_trace, sh.W, p->lde.as<uint32_t>()));
        // the row layout: next rows (LDE row j + 2 = the point g x_j) and the selectors at x_j behind the W1 columns
        if (sh.rf)
            TRY(row_layout_columns(p->lde.as<uint32_t>(), sh.N, sh.logN, sh.W1, p->d_next_cols, (uint32_t)p->h_next_cols.size(), 2,
                                   (sh.rf & kRowsSelector) != 0, false));
        return 0;
    }));
    TRY(commit_mixed(s, [&](size_t a, const uint32_t*& m, uint32_t& w) {
        m = s.sbv[a] ? s.coef_first(a) : s.prover(a)->lde.as<uint32_t>();
        w = s.sh[a].W;
    }, 0, root));
    PW_HIP_TRY(hipStreamSynchronize(s.st));
    s.pf.root(root);
    return 0;
}

// LogUp permutation matrices (shared challenges straight from the segment transcript), one mixed tree; al and the sums S[a] out
int commit_logup(Seg& s, bb::Ext& al, std::vector<bb::Ext>& S) {
    const size_t A = s.A;
    uint32_t root[8];
    al = s.pf.ch.sample_ext();
    const bb::Ext bl = s.pf.ch.sample_ext();
    std::vector<const uint32_t*> sp;
    TRY(s.fan.each(A, [&](size_t a) -> int {
        PwProver* p = s.prover(a);
        const AirBufs B = s.bufs_of(a);
        TRY(ext_powers(bl, p->max_args + 2, false, false, B.blpow));  // beta^0 .. (computed where they are used: no upload per AIR)
        const uint32_t* s_words[4];  // S = phi(last row); a streamed AIR's is parked in its gbuf (free until the DEEP stage)
        TRY(logup_stage(p, s.sh[a], s.mode_of(a), s.Lc[a], B, al, s_words));
        sp.insert(sp.end(), s_words, s_words + 4);
        return 0;
    }));
    TRY(commit_mixed(s, [&](size_t a, const uint32_t*& m, uint32_t& w) {
        m = s.sbv[a] ? s.prover(a)->perm.as<uint32_t>() : s.prover(a)->plde.as<uint32_t>();  // (streamed: the coefficient arrays)
        w = s.sh[a].Wp;
    }, 2, root));
    PW_HIP_TRY(hipMemcpyAsync(s.m.sptrs, sp.data(), sp.size() * 8, hipMemcpyHostToDevice, s.st));
    TRY(gather_words(s.m.sptrs, (uint32_t)sp.size(), s.m.small));
    std::vector<uint32_t> sw(4 * A);
    PW_HIP_TRY(hipMemcpyAsync(sw.data(), s.m.small, sw.size() * 4, hipMemcpyDeviceToHost, s.st));
    PW_HIP_TRY(hipStreamSynchronize(s.st));  // (sp and sw are locals)
    s.pf.root(root);
    for (size_t a = 0; a < A; ++a) {
        for (int k = 0; k < 4; ++k) S[a].c[k] = sw[4 * a + k];
        s.pf.ext(S[a]);
    }
    return 0;
}

// quotients (shared alpha), one mixed tree over the 8-column chunk matrices
int commit_quotient(Seg& s, bb::Ext al, const std::vector<bb::Ext>& S) {
    uint32_t root[8];
    const bb::Ext alpha = s.pf.ch.sample_ext();
    TRY(s.fan.each(s.A, [&](size_t a) -> int {
        const AirBufs B = s.bufs_of(a);
        TRY(ext_powers(alpha, s.sh[a].M, true, false, B.apow));  // alpha^(M - 1) .. alpha^0
        return quotient_stage(s.prover(a), s.sh[a], s.mode_of(a), s.Lc[a], B, al, S[a]);
    }));
    TRY(commit_mixed(s, [&](size_t a, const uint32_t*& m, uint32_t& w) { m = s.prover(a)->qlde.as<uint32_t>(); w = 8; }, 1, root));
    PW_HIP_TRY(hipStreamSynchronize(s.st));
    s.pf.root(root);
    return 0;
}

// ---- openings: per AIR main | preprocessed | perm at zeta | quotient | perm at g zeta [| main | preprocessed at g zeta] ------------
// all AIRs' values fetched with one copy
int open_all(Seg& s, bb::Ext zeta, std::vector<bb::Ext>& gzeta, std::vector<bb::Ext>& opened) {
    TRY(s.fan.each(s.A, [&](size_t a) -> int {
        gzeta[a] = bb::ext_scale(zeta, field::root_of_unity((int)s.sh[a].log_h));
        const uint32_t whole[2] = {0, s.sh[a].Wp};  // the permutation matrix in one piece: the values are fetched after the join
        return open_stage(s.prover(a), s.sh[a], s.mode_of(a), s.bufs_of(a), zeta, gzeta[a], s.m.opened + s.y.koff[a], whole, 1, [] { return 0; });
    }));
    opened.resize(s.y.K_total);
    PW_HIP_TRY(hipMemcpyAsync(opened.data(), s.m.opened, s.y.K_total * sizeof(bb::Ext), hipMemcpyDeviceToHost, s.st));
    PW_HIP_TRY(hipStreamSynchronize(s.st));
    for (const bb::Ext& e : opened) s.pf.ext(e);
    return 0;
}

// ---- reduced openings per height: the tallest into FRI's first layer, the smaller heights into their vectors behind the layers ----
int reduce_openings(Seg& s, bb::Ext zeta, const std::vector<bb::Ext>& gzeta, const std::vector<bb::Ext>& opened) {
    const SegLayout& y = s.y;
    const bb::Ext gamma = s.pf.ch.sample_ext();
    std::vector<bb::Ext> gpow(y.K_total);
    { bb::Ext g = bb::ext_one(); for (auto& x : gpow) { x = g; g = bb::ext_mul(g, gamma); } }
    // the DEEP kernels take the powers as CENTRED representatives (signed 64-bit accumulation, bb::ExtCentredAcc); the host sums
    // below use the canonical ones
    std::vector<bb::Ext> gpow_c(gpow);
    for (auto& e : gpow_c) for (auto& c : e.c) c = (uint32_t)bb::centred(c);
    PW_HIP_TRY(hipMemcpyAsync(s.m.gpow, gpow_c.data(), y.K_total * sizeof(bb::Ext), hipMemcpyHostToDevice, s.st));
    std::vector<char> started(y.L + 1, 0);
    for (size_t a = 0; a < s.A; ++a) {
        const AirShape& sh = s.sh[a];
        const size_t k0 = y.koff[a];
        bb::Ext sum1 = bb::ext_zero(), sum2 = bb::ext_zero();
        auto sums = [&]() {
            for (size_t k = 0; k < sh.K1; ++k) sum1 = bb::ext_add(sum1, bb::ext_mul(gpow[k0 + k], opened[k0 + k]));
            for (size_t k = sh.K1; k < sh.K; ++k) sum2 = bb::ext_add(sum2, bb::ext_mul(gpow[k0 + k], opened[k0 + k]));
        };
        bb::Ext* target = sh.logN == y.L ? s.d_v : s.d_v + y.ro_off[sh.logN];
        bb::Ext* out = started[sh.logN] ? s.d_v + y.tmp_off : target;
        TRY(deep_stage(s.prover(a), sh, s.mode_of(a), s.Lc[a], s.bufs_of(a), s.m.gpow + k0, gamma, sums, sum1, sum2, zeta, gzeta[a], out));
        if (started[sh.logN]) TRY(ext_axpy(target, nullptr, out, sh.N));
        started[sh.logN] = 1;
    }
    PW_HIP_TRY(hipStreamSynchronize(s.st));  // gpow_c is a local
    return 0;
}

// ---- queries -------------------------------------------------------------------------------------------------------------------
uint32_t phase_width(const AirShape& sh, int ph) { return ph == 0 ? sh.W : ph == 1 ? sh.Wp : 8u; }

// The query phase: the rows of every tree, the preprocessed rows, the siblings' offsets, the answers to the host, their emission
int answer_queries(Seg& s) {
    const SegLayout& y = s.y;
    const size_t A = s.A;
    const uint32_t nq = y.nq;
    const int L = y.L;
    std::vector<uint32_t> qs(nq), idx(A * nq);
    for (auto& q : qs) q = s.pf.ch.sample_bits(L);
    for (size_t a = 0; a < A; ++a)
        for (uint32_t i = 0; i < nq; ++i) idx[a * nq + i] = qs[i] & (uint32_t)(s.sh[a].N - 1);
    PW_HIP_TRY(hipMemcpyAsync(s.m.idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice, s.st));
    // rows: tree by tree (proof order main, perm, quotient), AIR by AIR, nq rows each
    std::vector<size_t> row_off[3], pre_row_off(A, 0), pre_dig_off(A, 0);
    std::vector<GatherRowsJob> jobs;  // (alive until the synchronisation below)
    size_t ro = 0;
    TRY(s.fan.fork());  // after the index upload
    for (int ph = 0; ph < 3; ++ph) {
        if (ph == 1 && !s.lg) continue;
        row_off[ph].resize(A);
        for (size_t a = 0; a < A; ++a) {
            PwProver* p = s.prover(a);
            const uint32_t* m = ph == 0 ? p->lde.as<uint32_t>() : ph == 1 ? p->plde.as<uint32_t>() : p->qlde.as<uint32_t>();
            const uint32_t w = phase_width(s.sh[a], ph);
            row_off[ph][a] = ro;
            s.fan.on_air(a);
            if (s.sbv[a] && ph != 2) {
                // streamed: the rows are rebuilt from the coefficient arrays (index scratch: the AIR's own gbuf, free by now)
                uint32_t* d_scr = p->gbuf.as<uint32_t>();
                TRY(streamed::query_rows(s.sctx(a), ph == 0 ? s.tcoef_of(a) : p->perm.as<uint32_t>(), w, idx.data() + a * nq, nq, d_scr, d_scr + nq,
                                         s.m.rows + ro));
            } else {
                jobs.push_back(GatherRowsJob{m, (uint64_t)s.sh[a].N, w, (uint32_t)(a * nq), (uint64_t)ro});
            }
            ro += (size_t)nq * w;
        }
    }
    TRY(s.fan.join());
    // the preprocessed rows (the fixed LDE the prover keeps) go into the same launch; their siblings come from each AIR's own tree
    std::vector<uint64_t> pre_offs;
    for (size_t a = 0; a < A; ++a) {
        const AirShape& sh = s.sh[a];
        if (!sh.Wf) continue;
        pre_row_off[a] = ro;
        jobs.push_back(GatherRowsJob{s.prover(a)->pre_lde.as<uint32_t>(), (uint64_t)sh.N, sh.Wf, (uint32_t)(a * nq), (uint64_t)ro});
        ro += (size_t)nq * sh.Wf;
        pre_dig_off[a] = pre_offs.size();
        for (uint32_t qi = 0; qi < nq; ++qi)
            for (int l = 0; l < sh.logN; ++l) {
                const size_t size = sh.N >> l, p = qs[qi] & (size - 1);
                pre_offs.push_back(merkle_level_offset(sh.N, l) + (((p + size / 2) & (size - 1)) * 8));
            }
    }
    if (!jobs.empty()) {  // the resident matrices' rows: one launch for all AIRs and trees
        PW_HIP_TRY(hipMemcpyAsync(s.m.jobs, jobs.data(), jobs.size() * sizeof(GatherRowsJob), hipMemcpyHostToDevice, s.st));
        TRY(gather_rows_multi(s.m.jobs, (uint32_t)jobs.size(), gather_rows_max_width(jobs.data(), jobs.size()), s.m.idx, nq, s.m.rows));
    }
    // the mixed trees' siblings (digest arena order: main | quotient | perm), then the FRI part, query by query
    const int tree_of_phase[3] = {0, 2, 1};
    std::vector<uint64_t> dig_offs, ext_offs;
    for (uint32_t qi = 0; qi < nq; ++qi) {
        const size_t q = qs[qi];
        for (int ph = 0; ph < 3; ++ph) {
            if (ph == 1 && !s.lg) continue;
            const size_t base = (size_t)tree_of_phase[ph] * y.tree_words;
            for (int l = 0; l < L; ++l) {
                const size_t size = y.Nmax >> l, p = q & (size - 1);
                dig_offs.push_back(base + merkle_level_offset(y.Nmax, l) + (((p + size / 2) & (size - 1)) * 8));
            }
        }
        fri_query_offsets(q, L, y.fri, (size_t)y.n_trees * y.tree_words, ext_offs, dig_offs);
    }
    const size_t nd = dig_offs.size(), ne = ext_offs.size(), npd = pre_offs.size();
    if (nd + npd > y.n_dig) return (int)hipErrorInvalidValue;
    // the answers leave the device as canonical words; the rows' copy ends with the digests'
    TRY(canonicalize_words(s.m.rows, ro));
    std::vector<uint32_t> rows(ro + 1), dig, ext;
    PW_HIP_TRY(hipMemcpyAsync(rows.data(), s.m.rows, ro * 4, hipMemcpyDeviceToHost, s.st));
    auto preprocessed_digests = [&]() -> int {  // (after the mixed trees' siblings in dig_out)
        uint64_t* d_pre_offs = s.m.offs + nd + ne;
        if (npd) PW_HIP_TRY(hipMemcpyAsync(d_pre_offs, pre_offs.data(), npd * 8, hipMemcpyHostToDevice, s.st));
        for (size_t a = 0; a < A; ++a)
            if (s.sh[a].Wf)
                TRY(gather_records(s.prover(a)->pre_tree.as<uint32_t>(), d_pre_offs + pre_dig_off[a], 8u, nq * (uint32_t)s.sh[a].logN,
                                   s.m.dig_out + (nd + pre_dig_off[a]) * 8));
        return 0;
    };
    TRY(fetch_query_answers(s.d_dig, s.d_v, dig_offs, ext_offs, s.m.offs, s.m.dig_out, s.m.ext_out, npd, preprocessed_digests, dig, ext));
    s.pf.words.reserve(s.pf.words.size() + nq + ro + nd * 8 + ne * 4);
    size_t dpos = 0, epos = 0;
    for (uint32_t qi = 0; qi < nq; ++qi) {
        s.pf.put(qs[qi]);
        for (int ph = 0; ph < 3; ++ph) {
            if (ph == 1 && !s.lg) continue;
            for (size_t a = 0; a < A; ++a) {
                const uint32_t w = phase_width(s.sh[a], ph);
                s.pf.put_raw(&rows[row_off[ph][a] + (size_t)qi * w], w);
            }
            s.pf.put_raw(&dig[dpos * 8], (size_t)L * 8);
            dpos += L;
            if (ph != 0) continue;
            // after the main tree's answer: each preprocessed row and its path in that AIR's own tree
            for (size_t a = 0; a < A; ++a) {
                const AirShape& sh = s.sh[a];
                if (!sh.Wf) continue;
                s.pf.put_raw(&rows[pre_row_off[a] + (size_t)qi * sh.Wf], sh.Wf);
                s.pf.put_raw(&dig[(nd + pre_dig_off[a] + (size_t)qi * sh.logN) * 8], (size_t)sh.logN * 8);
            }
        }
        put_fri_answer(s.pf, L, dig, ext, dpos, epos);
    }
    return 0;
}

// ---- the protocol ----------------------------------------------------------------------------------------------------------------
int prove_segment_impl(const PwSegmentAir* airs, size_t A, int logup_flag, bool honour_flags, const uint32_t** proof_words, size_t* n_words) {
    if (!airs || !A || !proof_words || !n_words) return (int)hipErrorInvalidValue;
    const bool lg = logup_flag != 0;
    std::vector<char> handed;
    std::vector<int> by_air;
    TRY(validate_airs(airs, A, lg, honour_flags, handed));
    TRY(forced_modes_by_air(A, by_air));
    (void)hipGetLastError();
    TRY(poseidon2_upload_params());
    {   // run-time specialised expression kernels of all AIRs that qualify, compiled in one concurrent batch (prover_jit.hip)
        std::vector<PwProver*> ps(A);
        std::vector<uint32_t> lhs(A);
        for (size_t a = 0; a < A; ++a) { ps[a] = airs[a].prover; lhs[a] = airs[a].log_height; }
        (void)specialise_provers(ps.data(), A, lhs.data(), false);
    }
    SegCtx& cx = g_ctx;
    cx.pub_snapshot.assign(A, {});
    for (size_t a = 0; a < A; ++a) cx.pub_snapshot[a] = airs[a].prover->h_pub;
    Seg s(airs, A, lg, std::move(handed), cx, stream());
    TRY(s.fan.open(A));

    // buffers: the segment's own arenas (every byte from the layout), then per AIR what its mode needs
    TRY(cx.dig.ensure(s.y.dig_bytes));
    TRY(cx.inject.ensure(s.y.inject_bytes));
    TRY(cx.ext.ensure(s.y.ext_bytes));
    TRY(cx.misc.ensure(s.y.misc_bytes));
    s.d_dig = cx.dig.as<uint32_t>();
    s.d_v = cx.ext.as<bb::Ext>();
    s.m = carve_misc(s.y, cx.misc.as<uint8_t>());
    choose_modes(s, by_air);
    for (size_t a = 0; a < A; ++a) {
        if (s.sbv[a]) TRY(ensure_proof_buffers(s.prover(a), s.sh[a].log_h, s.sbv[a], s.Lc[a], s.eat[a] != 0));
        else TRY(ensure_air(s.prover(a), s.sh[a], s.Lc[a]));
    }
    TRY(write_header(s));

    bb::Ext al = bb::ext_zero();
    std::vector<bb::Ext> S(A, bb::ext_zero()), gzeta(A), opened;
    TRY(commit_main(s));
    if (lg) TRY(commit_logup(s, al, S));
    TRY(commit_quotient(s, al, S));
    const bb::Ext zeta = s.pf.ch.sample_ext();
    TRY(open_all(s, zeta, gzeta, opened));
    TRY(reduce_openings(s, zeta, gzeta, opened));

    // FRI over the unshifted subgroups, the smaller heights rolled in as their size is reached
    TRY(fri_commit_phase(s.pf, s.y.fri, s.y.L, s.d_v, s.d_dig + s.y.n_trees * s.y.tree_words, bb::R_MOD_P, [&](int l, const bb::Ext& beta, bb::Ext* nv, size_t n) {
        const int lk = s.y.L - l - 1;
        if (lk < 2 || !s.y.has_height[lk]) return 0;
        const bb::Ext beta2 = bb::ext_mul(beta, beta);
        return ext_axpy(nv, &beta2, s.d_v + s.y.ro_off[lk], n);
    }));
    uint32_t witness = 0;
    TRY(grind(s.pf.ch, s.cfg.pow_bits, s.m.small, &witness));
    s.pf.put(witness);
    if (s.y.nq) TRY(answer_queries(s));

    *proof_words = s.pf.words.data();
    *n_words = s.pf.words.size();
    return (int)hipGetLastError();
}

}  // namespace

extern "C" int pw_prove_segment(const PwSegmentAir* airs, size_t n_airs, int logup_flag, const uint32_t** proof_words, size_t* n_words) {
    return prove_segment_impl(airs, n_airs, logup_flag, false, proof_words, n_words);
}

extern "C" int pw_prove_segment_consuming(const PwSegmentAir* airs, size_t n_airs, int logup_flag, const uint32_t** proof_words, size_t* n_words) {
    return prove_segment_impl(airs, n_airs, logup_flag, true, proof_words, n_words);
}

// the bytes of the calling thread's LAST segment proof's plan: with all AIRs resident | as chosen | what the policy had to work with
// (all 0 when no policy ran: forced modes, no device information)
extern "C" void pw_segment_last_plan(size_t* resident_bytes, size_t* planned_bytes, size_t* available_bytes) {
    if (resident_bytes) *resident_bytes = g_ctx.last_plan[0];
    if (planned_bytes) *planned_bytes = g_ctx.last_plan[1];
    if (available_bytes) *available_bytes = g_ctx.last_plan[2];
}

// the mode the AIRs of the calling thread's LAST segment proof ran in: out[a] = log2 of the number of sub-cosets (0 = resident),
// + 0x100 when the trace was overwritten by its coefficient arrays (pw_trace_from_coefficients restores it); out may be NULL (count only)
extern "C" size_t pw_segment_last_modes(uint32_t* out, size_t cap) {
    const std::vector<uint32_t>& m = g_ctx.last_modes;
    for (size_t a = 0; out && a < m.size() && a < cap; ++a) out[a] = m[a];
    return m.size();
}

// device bytes the calling thread's segment context holds (the mixed trees, injected digests, FRI layers, tables, parked sponge states):
// with pw_prover_device_bytes of its provers, what a segment proof keeps allocated after the call
extern "C" size_t pw_segment_context_bytes(void) { return g_ctx.bytes(); }

// ---- test hooks (not declared in include/: the CPU tests of the memory policy) ----------------------------------------------------
// pw::plan_segment_streams on caller-made tables (streamed: n x 5; b_max: 0 = may not stream); returns the bytes planned
extern "C" size_t pw_segment_stream_plan(size_t n, const size_t* resident, const size_t* streamed, const int* b_max, size_t own, size_t avail,
                                         int* sbv) {
    return pw::plan_segment_streams(n, resident, streamed, b_max, own, avail, sbv);
}

// the tables the calling thread's last segment proof planned with (empty when no policy ran: forced modes, no device information);
// returns the number of AIRs, fills up to cap of them
extern "C" size_t pw_segment_last_plan_tables(size_t* resident, size_t* streamed, int* b_max, size_t cap) {
    const SegCtx& cx = g_ctx;
    const size_t n = cx.plan_resident.size();
    for (size_t a = 0; a < n && a < cap; ++a) {
        if (resident) resident[a] = cx.plan_resident[a];
        if (b_max) b_max[a] = cx.plan_b_max[a];
        for (int b = 0; streamed && b < 5; ++b) streamed[a * 5 + b] = cx.plan_streamed[a * 5 + b];
    }
    return n;
}
