/*
 * powdr_prover.h — C ABI of the MI355X STARK prover ("pw-stark v0") in libpowdr_gpu.
 *
 * Boundary B2. The reference reaches its prover through the Rust
 * trait seam `StarkEngine::prove(pk, ProvingContext{per_trace: [(air_id,
 * AirProvingContext{cached_mains, common_main, public_values})]})`:
 *   call sites  /root/reference/openvm/src/trace_generation.rs:97-139 (callback(seg_idx, vm, pk, ctx)),
 *               /root/reference/openvm-riscv/src/lib.rs:327-341 (sdk.app_prover(exe).prove + verify_app_proof)
 *   engines     /root/reference/openvm/src/lib.rs:69-95 (BabyBearPoseidon2CpuEngine / ...GpuEngine)
 *   the AIR     /root/reference/openvm/src/powdr_extension/chip.rs:94-130 (PowdrAir::eval: current-row
 *               constraints `assert_zero(expr)`, no public values of its own (system AIRs have them: pw_prover_create_public below), no cached/preprocessed trace; the periphery
 *               chips that receive its lookups DO keep their tables in preprocessed columns — segment proofs take
 *               those through pw_prover_create_preprocessed, "pw-stark v1 + preprocessed" below)
 * The trait's method list lives in the un-vendored `openvm-stark-backend` crate, so this
 * header is the plain-C surface a third engine `E` (beside the CPU and CUDA engines) would
 * call from its `prove`: one AIR = one prover object built from the AIR's constraint
 * programs (what keygen extracts from `PowdrAir::eval` through the symbolic builder), and
 * `pw_prover_prove` consumes the AirProvingContext's `common_main` as a column-major
 * device matrix — exactly what `PowdrChipGpu::generate_proving_ctx` returns
 * (/root/reference/openvm/src/powdr_extension/trace_generator/cuda/mod.rs:404-421).
 *
 * All `d_` pointers are device pointers owned by the caller. Field words are BabyBear in
 * Montgomery form on the device; proof words are canonical u32 (little endian).
 * Return value 0 = success, otherwise a hipError_t (or -1 for malformed arguments).
 */
#ifndef POWDR_PROVER_H
#define POWDR_PROVER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PwProver PwProver;

typedef struct {
    uint32_t num_queries; /* FRI queries (blow-up is fixed at 2: constraint degree <= 3) */
    uint32_t pow_bits;    /* proof-of-work bits before the query phase, 0 = none */
} PwStarkConfig;

/* Constraint programs: post-fix bytecode with the trace-generation opcodes
 * (PUSH_APC=0 with a COLUMN INDEX operand, PUSH_CONST=1, ADD=2, SUB=3, MUL=4, NEG=5),
 * spans = {off, len} pairs in u32 words. Host pointers; copied. Returns NULL for a malformed program — a span past the bytecode, an
 * unknown opcode, an unbalanced or too deep stack, a column index >= width (the same for pw_prover_create_logup's interaction
 * programs) — and when the device tables cannot be allocated. */
PwProver* pw_prover_create(const PwStarkConfig* cfg, uint32_t width, const uint32_t* cons_bytecode,
                           size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints);
/* The same AIR including its bus interactions (PowdrAir::eval's `push_interaction`, chip.rs:117-129), proven
 * with committed LogUp columns ("pw-stark v0 + LogUp", oracle/stark_oracle.cpp): interactions = n x {bus id,
 * n_args, first span index}, spans = {off,len} pairs laid out [mult, arg0, arg1, ...] per interaction into
 * `inter_bytecode` (post-fix, column-index operands) — i.e. powdr_apc_compile_bus(apc, 1, ...). The proof then
 * also carries the permutation-matrix commitment, the cumulative sum S and the extra openings. */
PwProver* pw_prover_create_logup(const PwStarkConfig* cfg, uint32_t width, const uint32_t* cons_bytecode,
                                 size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints,
                                 const uint32_t* interactions, size_t n_interactions, const uint32_t* inter_spans,
                                 size_t n_inter_spans, const uint32_t* inter_bytecode, size_t inter_bytecode_len);
/* LogUp across the AIRs of a segment: the challenges of the bus argument are drawn from the 8-word `bus seed`
 * alone, so every AIR proven with the same seed uses the same pair and the per-AIR cumulative sums add up.
 * Flow: pw_prover_trace_root for every AIR -> seed = a digest over all roots (the caller's choice; the segment
 * verifier must recompute it) -> pw_prover_set_bus_seed + pw_prover_prove per AIR. Without a seed (NULL, the
 * default) an AIR uses its own trace root. Canonical words. */
int pw_prover_trace_root(PwProver* p, const uint32_t* d_trace, uint32_t log_height, uint32_t* root8);
int pw_prover_set_bus_seed(PwProver* p, const uint32_t* seed8);
/* How the LogUp kernels evaluate this AIR's multiplicities and arguments: 0 = no LogUp extension, 1 = the bytecode
 * interpreter, 2 = "small forms" (k0 + k1 A + k2 B + k3 A B over at most two columns — fixed code; what the interactions of
 * optimised APCs look like; the few wider expressions of such an AIR still go through the interpreter). Chosen when at least
 * half of the expressions are small forms; POWDR_LOGUP_INTERPRET=1 at creation forces 1 (tests). */
int pw_prover_logup_path(const PwProver* p);
void pw_prover_destroy(PwProver* p);

/* ---- preprocessed (fixed) columns: "pw-stark v1 + preprocessed"  --------------------------------------------------
 * An AIR whose tables the proving key fixes (the periphery chips' VariableRangeCheckerAir, BitwiseOperationLookupAir<8>,
 * RangeTupleCheckerAir<2>, openvm/src/powdr_extension/trace_generator/cuda/periphery.rs:33-85): `pre_width` fixed
 * columns at height 2^log_height, d_pre = the fixed matrix (device, column-major, Montgomery; copied). In the constraint and
 * interaction programs an operand c < width is main column c, width <= c < width + pre_width is preprocessed column c - width — every
 * check of the programs (NULL for a malformed one, pw_prover_max_constraint_degree, pw_jit_compile_check with width + pre_width as the
 * width) uses that combined bound. Other arguments as pw_prover_create_logup; interactions == NULL: a constraints-only AIR (proven in
 * segments with logup = 0), n_interactions = 0 with tables: an AIR of a LogUp segment without interactions. At creation the prover
 * extends and commits the fixed matrix once and keeps it, its LDE and its tree (counted by pw_prover_device_bytes).
 * Such a prover proves in segments only, at exactly 2^log_height rows (pw_prove_segment / _consuming; another height: -1), always with
 * its extension resident (never streamed, whatever POWDR_STREAM_LOG_BLOCKS* say; pw_segment_last_modes reports 0); pw_prover_prove,
 * pw_prover_prove_consuming, pw_prover_trace_root and pw_prove_airs return -1. pw_prover_check_constraints reads operands >= width from
 * the fixed matrix. The proof of a segment with at least one such AIR carries magic PWS4. */
PwProver* pw_prover_create_preprocessed(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                        const uint32_t* d_pre, const uint32_t* cons_bytecode, size_t bytecode_len,
                                        const uint32_t* cons_spans, size_t n_constraints, const uint32_t* interactions,
                                        size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                                        const uint32_t* inter_bytecode, size_t inter_bytecode_len);
/* The preprocessed commitment (8 canonical words): the verifying key's part, PwAirPreprocessed::root8. -1: no preprocessed columns. */
int pw_prover_preprocessed_root(const PwProver* p, uint32_t* root8);
uint32_t pw_prover_preprocessed_width(const PwProver* p); /* 0: none */

/* ---- next-row operands and row selectors: "pw-stark v1 + rows"  --------------------------------------------------
 * An AIR whose constraints read the next row or Plonky3's row selectors (OpenVM's `main.row_slice(1)`, `when_first_row()`,
 * `when_transition()`; powdr's OpenVmReference::{WitnessColumn(_, next), IsFirstRow, IsLastRow, IsTransition}). With W1 = width +
 * pre_width, an operand c of a CONSTRAINT program is
 *     c < W1             main (c < width) or preprocessed column c on the current row, as pw_prover_create_preprocessed;
 *     W1 <= c < 2 W1     column c - W1 on the NEXT row (the row after the last is row 0);
 *     2 W1               is_first_row  = Z_H(x) / (x - 1)      (H at row 0, 0 elsewhere on the trace domain)
 *     2 W1 + 1           is_last_row   = Z_H(x) / (x - g^-1)   (H g at row H - 1, 0 elsewhere)
 *     2 W1 + 2           is_transition = x - g^-1              (g^j - g^-1 at row j)
 * Degrees (Plonky3's degree_multiple): a column of either row and the first / last row selectors 1, is_transition 0; every constraint
 * at most 3 (pw_prover_max_constraint_degree reports by this rule). INTERACTION operands stay below W1 (current-row columns only).
 * NULL for an operand outside these bounds, a constraint of degree > 3 or a malformed program. pre_width = 0: no fixed matrix
 * (log_height, d_pre unused; any height >= 2 rows); pre_width > 0: as pw_prover_create_preprocessed. Other arguments as there.
 * An AIR is ROW-AWARE if one of its constraint programs reads an operand >= W1, TWO-POINT if one reads a next-row operand
 * (pw_prover_row_flags: bit 0 two-point, bit 1 reads a selector; 0: neither — the prover then proves exactly as the plain or
 * preprocessed one). Such a prover proves in segments only (pw_prove_segment / _consuming); pw_prover_prove, _prove_consuming,
 * _trace_root and pw_prove_airs return -1. A row-aware AIR is never streamed (pw_segment_last_modes reports 0). The proof of a segment
 * with at least one row-aware AIR carries magic PWS5; other segments keep their PWS3 / PWS4 words.
 * pw_prover_check_constraints reads the next row as (j + 1) mod H and the selectors' exact values on the trace domain (heights up to
 * 2^26 rows, the segment limit; above: -1). */
PwProver* pw_prover_create_transition(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                      const uint32_t* d_pre, const uint32_t* cons_bytecode, size_t bytecode_len,
                                      const uint32_t* cons_spans, size_t n_constraints, const uint32_t* interactions,
                                      size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                                      const uint32_t* inter_bytecode, size_t inter_bytecode_len);
uint32_t pw_prover_row_flags(const PwProver* p);

/* ---- public values: "pw-stark v1 + public values"  --------------------------------------------------------------
 * An AIR with PUBLIC VALUES (Plonky3's `builder.public_values()`, OpenVM's `AirProvingContext.public_values`): field elements that are
 * part of the statement, known to prover and verifier, fixed per proof and not when the prover is made. With W1 = width + pre_width, in a
 * CONSTRAINT program operand 2 W1 + 3 + k, k < n_public <= 256, is public value k (behind the row layout of pw_prover_create_transition,
 * whether or not the AIR is row-aware); its degree is 0, like is_transition, and the bound of 3 stays. INTERACTION operands stay below W1.
 * NULL for an operand at or above 2 W1 + 3 + n_public, n_public > 256, a constraint of degree > 3, a malformed program. Every other
 * argument as pw_prover_create_transition; with n_public = 0 the prover IS a pw_prover_create_transition prover (same proof words).
 * pw_prover_row_flags is derived as there, from the operands in [W1, 2 W1 + 3): an AIR may have public values with row flags 0.
 * The values are not columns: they live in a small device array that every expression kernel receives as an argument and reads at the
 * (wave-uniform) index the program carries; the programs, the generated kernels and their on-disk cache key never depend on them.
 * pw_prover_set_public_values: `values` = n host words, canonical; -1 when n != n_public or a word is >= p. The prover keeps a host
 * copy, so one prover serves segment after segment. A segment proof snapshots the values when the call begins and uploads the snapshot
 * on the calling thread's launch stream: setting new values after the call has returned never races with it.
 * A prover with n_public > 0 proves in segments only (pw_prover_prove, _prove_consuming, _trace_root, pw_prove_airs: -1), is never
 * streamed (pw_segment_last_modes reports 0; the memory plan counts it resident, as a row-aware AIR) and makes pw_prove_segment return
 * -1, before any GPU work, while its values have never been set — it does not prove with zeros in their place.
 * pw_prover_check_constraints reads public operands from the values set (-1: none set). The proof of a segment with at least one such
 * AIR carries magic PWS6 and, right after the header words, the values of every such AIR in AIR order (canonical words). */
PwProver* pw_prover_create_public(const PwStarkConfig* cfg, uint32_t width, uint32_t pre_width, uint32_t log_height,
                                  const uint32_t* d_pre, uint32_t n_public, const uint32_t* cons_bytecode, size_t bytecode_len,
                                  const uint32_t* cons_spans, size_t n_constraints, const uint32_t* interactions,
                                  size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                                  const uint32_t* inter_bytecode, size_t inter_bytecode_len);
uint32_t pw_prover_n_public(const PwProver* p);
int pw_prover_set_public_values(PwProver* p, const uint32_t* values, size_t n);

/* Prove one trace (column-major, width x 2^log_height, Montgomery words, device).
 * *proof_words points at host memory owned by the prover, valid until the next call. */
int pw_prover_prove(PwProver* p, const uint32_t* d_trace, uint32_t log_height, const uint32_t** proof_words,
                    size_t* n_words);

/* The same proof (the same words) of a trace the caller HANDS OVER — what the reference does with `common_main`: the
 * trace generator moves the matrix into the AirProvingContext and the engine owns it from there
 * (/root/reference/openvm/src/powdr_extension/trace_generator/cuda/mod.rs:404-421). The prover may then overwrite
 * d_trace: when the low-degree extension is resident it does not; when the proof is STREAMED (pw_prover_stream_log_blocks)
 * the trace's coefficient arrays replace the trace in place instead of living in a buffer of their own — at BASELINE
 * configs[2] (3 731 x 2^22 + 4 632 permutation columns) that is 62.6 GB, the difference between walking the extended
 * domain as 4 sub-cosets and as 2 (half the coefficient re-reads of every pass). Afterwards d_trace holds, per column,
 * H * (the coefficients) in bit-reversed order; pw_trace_from_coefficients turns that back into the trace (exact).
 * d_trace must be 16-byte aligned (hipErrorInvalidValue otherwise; pw_prover_prove takes any 4-byte aligned trace).
 * pw_prover_stream_log_blocks_consuming: the mode such a proof would run in with the memory free now. */
int pw_prover_prove_consuming(PwProver* p, uint32_t* d_trace, uint32_t log_height, const uint32_t** proof_words,
                              size_t* n_words);
int pw_prover_stream_log_blocks_consuming(const PwProver* p, uint32_t log_height);
/* In place: width columns of 2^log_height H-scaled bit-reversed coefficients (what a streamed pw_prover_prove_consuming
 * leaves) -> the values on the trace domain, natural row order, canonical Montgomery words. d_scratch: 2^13 words. */
int pw_trace_from_coefficients(uint32_t* d_coeffs, uint32_t width, uint32_t log_height, uint32_t* d_scratch); /* d_coeffs 16-byte aligned */

/* "Mock prover": evaluate every constraint on every row of the trace on the device and report violations —
 * the counterpart of the reference's `debug_proving_ctx` used by its `prove_mock` tests
 * (openvm-riscv/src/lib.rs:288-294). *n_violations = number of (row, constraint) pairs that are non-zero;
 * if any, *first_row / *first_constraint name the first one in row-major order. */
int pw_prover_check_constraints(PwProver* p, const uint32_t* d_trace, uint32_t log_height, uint64_t* n_violations,
                                uint64_t* first_row, uint32_t* first_constraint);

/* The other half of the mock prover: are the BUSES of a segment balanced, tuple by tuple — what `debug_proving_ctx`
 * checks besides the constraints — evaluated on the raw traces, nothing committed, and if not, WHICH tuples are left over.
 * A TUPLE is (bus, n_args, args...): two tuples are equal only when the bus, the number of arguments and every argument are equal,
 * the reference's rule (it compares the field vectors of the interactions). That is deliberately STRICTER than the LogUp sum of a
 * proof, in which (a, b) and (a, b, 0) have the same denominator: a sender of (a, b) and a receiver of (a, b, 0) verify with
 * check_balance and are reported here as two unbalanced tuples. A bus is balanced when for every tuple the multiplicities — over all
 * AIRs, interactions and rows, padding rows included; sends + m, receives - m as everywhere in this header — sum to 0 mod p.
 * Interactions are evaluated exactly as the prover evaluates them: current-row operands below width + pre_width, operands >= width
 * from the prover's fixed matrix (as pw_prover_check_constraints arranges it). A prover made without interaction tables contributes
 * nothing. Bus ids are compared mod p (as the provers hold them).
 *   airs / n_airs     as for pw_prove_segment (flags ignored; nothing is handed over; at most 2^18 AIRs of at most 2^20 interactions,
 *                     2^26 rows). A preprocessed prover at another height than its own, or one that occurs twice in the list: -1.
 *   buses / n_buses   the bus ids to check (duplicates count once); n_buses == 0: every bus id that occurs in the provers' tables.
 *   seed              the two challenges of pass A and of the fingerprints are derived from it. NOTHING reported depends on it.
 *   table_bytes       the most device bytes the tally table of ONE bus may take (40 per slot, a power of two of slots); 0: half of
 *                     what pw_get_device_budget / the free memory allow. A bus starts with 2^16 slots (2.6 MB) and is tallied again
 *                     into a table four times as large while it overflows, up to this bound (never beyond twice its active triples).
 *                     A table holds 7/8 of its slots in tuples (so that probing stays short): give a bus you know 8/7 of its
 *                     distinct tuples, rounded up to a power of two.
 *   flags             PW_BUS_CHECK_TALLY_ALL: run the tuple tally for the buses pass A found balanced too.
 *   summaries         one per checked bus, ordered by bus id; summary_cap smaller than their number: -1 (n_buses == 0: as many
 *                     as there are distinct ids; otherwise as many as distinct entries of `buses`). NULL with summary_cap 0: skipped.
 *   tuples            the unbalanced tuples ordered by (bus, n_args, args lexicographically on canonical words), truncated at
 *                     tuple_cap (n_unbalanced of the summaries keeps the full count). NULL with tuple_cap 0: skipped.
 * Pass A (always): per bus sum m / (alpha + sum_j beta^(j+1) a_j + beta^(n+1) n) over everything, in the extension field; zero
 * <=> balanced up to the soundness of LogUp itself (below 2^-90 for a bus of 2^26 tuples and a seed chosen independently of the traces:
 * DESIGN.md §5i). Pass B (unbalanced buses, or all): an exact tally per tuple in a device hash table keyed by the 124-bit fingerprint;
 * a bound too small for a bus — or a table the device cannot allocate — gives that bus status 2: never an error, never a wrong
 * answer, and (allocation failures apart) the same status every time for the same table_bytes. Where pass B
 * ran without overflowing, its verdict is the one reported. The sum of a tuple's centred multiplicities is kept in 64 bits: exact
 * for fewer than 2^33 contributions per tuple.
 * Nothing the caller or the provers own is modified (a preprocessed prover's staging copy of the trace is rewritten, as by a proof).
 * Stream contract as pw_prove_segment: the calling thread's launch stream; the call synchronises before it returns. Malformed
 * arguments return -1 before any GPU call. Scratch is per host thread: the table and the tuple lists are released before the call
 * returns, also when it returns an error; some twenty kilobytes of tables stay (pw_bus_check_scratch_bytes: held now; pw_bus_check_peak_bytes: the most the thread's last
 * call held at once), and every prover keeps 4 bytes per interaction (counted by pw_prover_device_bytes) from its first check on. */
#define PW_BUS_MAX_ARGS 16u
#define PW_BUS_CHECK_TALLY_ALL 1u   /* flags: run the tuple tally for balanced buses too (tests, statistics) */

typedef struct PwBusSummary {
    uint32_t bus;
    uint32_t status;         /* 0 balanced; 1 unbalanced, tuples listed; 2 unbalanced, tally table too small: not localised */
    uint64_t n_active;       /* (air, interaction, row) triples with a non-zero multiplicity on this bus */
    uint64_t n_unbalanced;   /* distinct tuples whose multiplicities do not sum to 0 mod p (0 when status is 0 or 2) */
} PwBusSummary;

typedef struct PwBusTuple {
    uint32_t bus, n_args;
    uint32_t args[PW_BUS_MAX_ARGS];  /* canonical words; the first 16 of a longer tuple (n_args keeps the real length) */
    uint32_t net_multiplicity;       /* canonical, non-zero: the sum of all multiplicities that carried this tuple */
    uint32_t air, interaction;       /* a witness: the lexicographically smallest (air, interaction, row) that contributed */
    uint64_t row;
    uint64_t n_contributions;
} PwBusTuple;

struct PwSegmentAir; /* below: "one segment = many AIRs" */
int pw_check_segment_buses(const struct PwSegmentAir* airs, size_t n_airs,
                           const uint32_t* buses, size_t n_buses,   /* n_buses == 0: every bus id that occurs */
                           uint64_t seed, size_t table_bytes,       /* 0: a default bounded by pw_get_device_budget / free memory */
                           uint32_t flags,
                           PwBusSummary* summaries, size_t summary_cap, size_t* n_summaries,
                           PwBusTuple* tuples, size_t tuple_cap, size_t* n_tuples);
size_t pw_bus_check_scratch_bytes(void);
size_t pw_bus_check_peak_bytes(void);

/* Verify a proof on the host (no GPU): the counterpart of the reference's CPU verification step
 * `verify_app_proof::<BabyBearPoseidon2CpuEngine>` (openvm-riscv/src/lib.rs:337-341). Constraint
 * programs as for pw_prover_create (post-fix, column-index operands, no INV_OR_ZERO).
 * Returns 0 = valid; 1 header, 2 constraint identity, 3 proof of work, 4 query index, 5 trace opening,
 * 6 quotient opening, 7 FRI layer, 8 final polynomial, 9 trailing words, 10 truncated/malformed,
 * 13 a proof word >= p (non-canonical encodings are rejected: proofs are not malleable). */
int pw_verify(const PwStarkConfig* cfg, uint32_t width, uint32_t log_height, const uint32_t* cons_bytecode,
              size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints, const uint32_t* proof_words,
              size_t n_words);

/* Verify a "pw-stark v0 + LogUp" proof (pw_prover_create_logup). Interaction arguments as for the prover.
 * Additional failure codes: 11 = permutation-matrix opening, 12 = the proof's bus seed is not
 * `expected_bus_seed` (NULL: not the proof's own trace root). On success `cumulative_sum` (4 canonical words,
 * may be NULL) receives this AIR's bus sum S = sum_rows sum_i m_i / d_i and `trace_root` (8 words, may be NULL)
 * its trace commitment; the caller accepts a segment when every proof verifies against the seed recomputed
 * from all the trace roots and the sums add up to zero (every send matched by a receive). */
int pw_verify_logup(const PwStarkConfig* cfg, uint32_t width, uint32_t log_height, const uint32_t* cons_bytecode,
                    size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints, const uint32_t* interactions,
                    size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                    const uint32_t* inter_bytecode, size_t inter_bytecode_len, const uint32_t* expected_bus_seed,
                    const uint32_t* proof_words, size_t n_words, uint32_t* cumulative_sum, uint32_t* trace_root);

/* How pw_prover_create_logup / pw_verify_logup pack the interactions into committed columns: consecutive
 * interactions share one extension column ("group") while the group's constraint keeps degree <= 3. Writes up to
 * `cap` group boundaries (interaction indices) to `out`, returns their number (n_groups + 1; 0 = malformed table).
 * The permutation matrix has 4 * (n_groups + 1) base columns. */
size_t pw_logup_group_starts(const uint32_t* interactions, size_t n_interactions, const uint32_t* inter_spans,
                             size_t n_inter_spans, const uint32_t* inter_bytecode, size_t inter_bytecode_len,
                             uint32_t* out, size_t cap);

/* ---- one segment = many AIRs -------------------------------------------------------------------------------------
 * The engine call the reference makes once per segment with all chips' traces, `engine.prove(pk, ProvingContext{
 * per_trace})` (openvm/src/trace_generation.rs:97-139, openvm-riscv/src/lib.rs:327-341). */
#define PW_AIR_HAND_OVER 1u /* PwSegmentAir::flags: the trace is the engine's to overwrite (pw_prove_segment_consuming) */
typedef struct PwSegmentAir {
    PwProver* prover;        /* one per AIR (pw_prover_create / _create_logup), reused from segment to segment */
    const uint32_t* d_trace; /* device, column-major width x 2^log_height, Montgomery */
    uint32_t log_height;
    uint32_t flags;          /* read by pw_prove_segment_consuming only (the struct's former padding: size and offsets unchanged) */
} PwSegmentAir;

/* ONE proof for all AIRs of the segment ("pw-stark v1", proof magic PWS3; protocol: oracle/stark_segment.inc) — the
 * shape of the reference's call: all matrices of a phase are committed in one mixed-height Poseidon2 tree, the openings of
 * all AIRs are reduced per height and checked by one FRI over the tallest domain, one query phase answers for everything.
 * logup != 0: every prover must come from pw_prover_create_logup (an AIR without interactions passes n_interactions = 0);
 * the bus challenges are drawn once from the segment transcript and the proof carries every AIR's cumulative sum.
 * Stream contract: the call runs on the calling thread's launch stream (powdr_gpu_set_stream), after everything the
 * caller enqueued there — trace generation included. *proof_words is owned by the library (per host thread) and valid
 * until that thread's next pw_prove_segment. Returns 0 or the first error. */
int pw_prove_segment(const PwSegmentAir* airs, size_t n_airs, int logup, const uint32_t** proof_words, size_t* n_words);

/* The same proof, same words, with the traces HANDED OVER per AIR (flags & PW_AIR_HAND_OVER) — the reference's chips move
 * `common_main` into the engine for every AIR of a segment (openvm/src/powdr_extension/trace_generator/cuda/mod.rs:404-421).
 * An AIR that is proven with its LDE resident leaves its trace alone; an AIR that is STREAMED (its extension does not fit beside
 * the others) keeps the coefficient arrays of a handed-over trace IN the caller's buffer instead of a copy of its own (configs[2]:
 * 62.6 GB, two sub-cosets instead of four). After the call such a buffer holds H-scaled bit-reversed coefficients
 * (pw_trace_from_coefficients restores the trace, exactly); handed-over traces must be 16-byte aligned (hipErrorInvalidValue).
 * pw_segment_last_modes: per AIR of the calling thread's last segment proof, log2(#sub-cosets) (0 = resident) | 0x100 if the
 * trace was overwritten; returns the number of AIRs. */
int pw_prove_segment_consuming(const PwSegmentAir* airs, size_t n_airs, int logup, const uint32_t** proof_words, size_t* n_words);
size_t pw_segment_last_modes(uint32_t* out, size_t cap);
/* The memory plan of the calling thread's last segment proof (bytes; zero when the modes were forced by POWDR_STREAM_LOG_BLOCKS or,
 * AIR by AIR, POWDR_STREAM_LOG_BLOCKS_BY_AIR):
 * with every AIR resident | as chosen | what the policy had to work with (free + held, head room, pw_set_device_budget). */
void pw_segment_last_plan(size_t* resident_bytes, size_t* planned_bytes, size_t* available_bytes);
/* Device bytes the calling thread's segment context holds now (mixed trees, injected digests, FRI layers, tables, parked sponge
 * states). After a segment proof, this + pw_prover_device_bytes of its provers is what the call left allocated: at most the
 * planned bytes of pw_segment_last_plan. */
size_t pw_segment_context_bytes(void);

/* ---- closing a segment's buses: the traces of the program and memory boundary AIRs ------------------------------
 * The receivers of the PC lookup and of the memory bus are AIRs like any other (powdr_amd/system_airs.py gives their programs);
 * their traces depend on everything the other AIRs send, and these two routines make them on the device from the other AIRs' raw
 * traces. Both take the AIR list of pw_check_segment_buses (same refusals: -1 before any GPU call), read the interactions on ONE bus
 * through the provers' own programs exactly as that check does (operands >= width from the prover's fixed matrix; a preprocessed
 * prover's staging copy of the trace is rewritten), modify nothing else of the caller's, run on the calling thread's launch stream
 * and synchronise before they return. Scratch is per host thread and released before the call returns, on every path, but for a
 * few kilobytes (pw_system_traces_scratch_bytes: held now; pw_system_traces_peak_bytes: the most the thread's last call held).
 *
 * pw_program_frequencies: d_freq_out[k] (2^log_h words, Montgomery) = the sum mod p of the multiplicities of all tuples on `bus`
 * that equal row k of the program table d_program (9 x 2^log_h, column-major, Montgomery: pc, opcode, a .. g), where
 * k = (pc - pc_base) / pc_step — the main column of the program AIR, which receives each row `freq` times. A tuple is FOREIGN when
 * its pc is below pc_base, not a multiple of pc_step away from it, past the table, when it has not nine arguments or differs from
 * its row in any word: foreign tuples are never dropped silently — *n_foreign counts them and *first_foreign (may be NULL) is the
 * one with the smallest (air, interaction, row), with its own multiplicity in net_multiplicity — and never counted in d_freq_out.
 * The sums are integer additions (64 bits: exact below 2^32 contributions per row), so the output does not depend on their order.
 *
 * pw_memory_boundary_trace: the trace of the memory boundary AIR — one row per touched location (as, ptr), sorted, 18 columns
 * [is_valid, as, ptr, p_lo, p_hi, init0..3, init_ts, fin0..3, fin_ts, same_as, d_lo, d_hi], column-major, 2^*log_height rows,
 * Montgomery, padding rows zero — from the tuples (as, ptr, four data words, timestamp) on `bus`: a location's initial words and
 * timestamp are those of the receive (multiplicity -1) with the smallest timestamp, its final ones those of the send (+1) with the
 * largest; ties go to the smallest (air, interaction, row), so the output does not depend on the order of arrival. An interaction
 * on `bus` that has not seven arguments: -1. d_trace_out holds 18 x 2^cap_log_height words; *log_height = ceil(log2 *n_locations),
 * at least 1. table_bytes bounds the address table (40 bytes per slot, grown from 2^16 slots by 4 while it overflows, full at 7/8,
 * as the tally table of pw_check_segment_buses; 0: half of what the device budget allows). *status: 0 = written; 1 = cap_log_height
 * too small (*n_locations and *log_height say what is needed); 2 = the table bound too small; 3 = a multiplicity on the bus that is
 * not +1 or -1; 4 = a location with only receives or only sends. With a status other than 0 nothing is written and 0 is returned.
 * The routine does NOT prove that memory was consistent — a read that returns what nobody wrote still gets its first receive and last
 * send paired up: run pw_check_segment_buses on the bus with the boundary AIR in the list afterwards (pass A is the cheap verdict,
 * pass B names the two tuples of a broken link). */
int pw_program_frequencies(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, uint32_t pc_base, uint32_t pc_step,
                           const uint32_t* d_program, uint32_t log_h, uint32_t* d_freq_out, uint64_t* n_foreign,
                           PwBusTuple* first_foreign);
int pw_memory_boundary_trace(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, size_t table_bytes, uint32_t* d_trace_out,
                             uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_locations, uint32_t* status);
size_t pw_system_traces_scratch_bytes(void);
size_t pw_system_traces_peak_bytes(void);
/* What the calling thread's last calls did. Of its last pw_memory_boundary_trace: the slots of the address table kept, the slots
 * occupied in it (= locations), the tables walked into (overflowed attempts included). Of its last call of either routine: rows x
 * interactions walked (an upper bound of the active triples). Of its last pw_program_frequencies: the additions asked for (active
 * triples), and the LDS and global atomics the kernel issued for them after merging. */
typedef struct PwSystemTraceStats {
    uint64_t table_slots, occupied_slots, tables, walked;
    uint64_t additions, lds_atomics, global_atomics;
} PwSystemTraceStats;
void pw_system_traces_last_stats(PwSystemTraceStats* out);
/* The first address table of the calling thread's later pw_memory_boundary_trace calls has 2^log_slots slots (6 .. 30; 0 = back to the
 * default, 2^16): a caller that knows its segment touches few locations starts small, one that knows it touches millions skips the
 * first growth steps. The result does not depend on it. -1: out of range. */
int pw_memory_boundary_set_start_slots(uint32_t log_slots);

/* ---- the Poseidon2 compression chip's trace (the AIR: powdr_amd/system_airs.py poseidon2_air) ----------------------
 * The contract of pw_memory_boundary_trace: `airs` is the AIR list of pw_check_segment_buses — the SENDERS on `bus`, not the chip —
 * with the same refusals (-1 before any GPU call; also for an interaction on `bus` that has not 24 arguments left[8], right[8], out[8]),
 * the call runs on the calling thread's launch stream and synchronises before it returns, scratch is released on every path.
 * The key is the 16 input words: every active (air, interaction, row) on `bus` adds its centred multiplicity to its key's 64-bit sum
 * in an open-addressing table (32 bytes per slot; keyed by a 124-bit fingerprint of the inputs as the tally of
 * pw_check_segment_buses; 2^start_log_slots slots at first, 6 .. 30, 0 = 2^16; grown by 4 while it overflows, full at 7/8, bounded
 * by table_bytes, 0 = half of what the device budget allows) and offers its packed witness to an atomic minimum. The `out` words of
 * the senders are NOT read: the chip computes the digest, and a sender with a wrong one gets its row and an unbalanced bus.
 * d_trace_out (307 x 2^cap_log_height words) receives 307 columns [mult | in[16] | cube, sbox[16] of full rounds 0..7 | pcube, psbox
 * of partial rounds 0..12 | out[8]], column-major, 2^*log_height rows (*log_height = ceil(log2 *n_rows), at least 1), Montgomery:
 * one row per distinct key, sorted by the key's smallest witness — every byte is independent of the order of arrival — with the
 * intermediates of the installed permutation (pw_set_poseidon2_constants) and mult = the sum mod p (a key whose multiplicities
 * cancel keeps its row with mult 0); padding rows are the row of the all-zero input with mult 0. *status: 0 = written; 1 =
 * cap_log_height too small (*n_rows and *log_height say what is needed); 2 = the table bound too small. With a status other than 0
 * nothing is written and 0 is returned. pw_system_traces_last_stats: table_slots, occupied_slots (= rows), tables, walked. */
int pw_poseidon2_compress_trace(const PwSegmentAir* airs, size_t n_airs, uint32_t bus, size_t table_bytes, uint32_t start_log_slots,
                                uint32_t* d_trace_out, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_rows,
                                uint32_t* status);

/* ---- empirical constraints: column ranges per pc and cell classes per basic block --------------------------------
 * The data-parallel half of the reference's `detect_empirical_constraints` (openvm/src/empirical_constraints.rs), on the instruction
 * AIRs' raw device traces. `airs` is the AIR list of pw_check_segment_buses; segment_of_air (n_airs words, NULL = all 0) says which
 * segment an entry's trace belongs to. An AIR without an interaction on `bus` (the execution bridge) is ignored. Of every other AIR
 * every row's interactions on `bus` are evaluated as the bus check evaluates them: all multiplicities 0 = padding, the row takes part
 * in nothing; otherwise exactly one interaction has the centred multiplicity -1 (the receive: its two arguments are the row's pc and
 * timestamp), every other non-zero one +1. Time key = segment << 32 | timestamp; cells = the canonical values of the AIR's `width`
 * main columns. `blocks`: start pcs strictly increasing, start + pc_step * n_instructions <= the next start.
 * Result (host side, canonical order: pcs and blocks ascending, a class's cells by (instruction, column), classes by first cell):
 *   per executed pc its 64-bit row count, the index of the AIR that executed it, and per column (lo, hi) = the elements n / 100 and
 *   n * 99 / 100 of the column's n values sorted as canonical integers (pw_empirical_percentile_indices);
 *   per listed block that ran (a head row and the n_instructions - 1 rows that follow it in time order, at the pcs start + k pc_step)
 *   the classes of at least two cells (instruction_idx, column_idx) that held equal values in EVERY instance the call saw.
 * Classes are found by 128-bit fingerprints and then VERIFIED cell against first cell over all instances; on a mismatch the grouping
 * is repeated under another seed, three times in all: the partition returned is exact, never probable.
 * The contract of the system-trace routines: the call runs on the calling thread's launch stream and synchronises before it
 * returns; scratch is per thread and released on every path. -1 before any GPU call: a NULL pointer, pc_step == 0, a block table that
 * is unsorted, overlapping or has a zero count, an AIR whose interactions on `bus` have not two arguments, 2^32 rows or more.
 * scratch_bytes bounds the scratch (0: half of what the device budget allows); the columns are walked in panels that fit.
 * *status: 0 = *out is set (pw_empirical_destroy frees it); 2 = the bound is too small for the row index or one column, *info = bytes
 * needed (before a row is read: as far as known then; a second status 2 is exact); 3 = not block-structured, *info = the smallest
 * time key of a head whose instructions do not follow it or of an in-block row without its head; 4 = two rows with one time key,
 * *info = the key; 5 = a pc executed by rows of two AIRs, *info = the pc; 6 = fingerprint collisions under every seed; 7 = a
 * multiplicity on the bus other than 0, +1, -1 or not exactly one receive in an active row, *info = air << 32 | row, the smallest.
 * Checked in the order 2 (the row index), 7, 4, 3, 5, 2 (one column), 6. With a non-zero status no result exists and 0 is
 * returned. */
typedef struct { uint32_t start_pc, n_instructions; } PwBasicBlock;
typedef struct PwEmpirical PwEmpirical;
int pw_empirical_detect(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, uint32_t pc_step,
                        const PwBasicBlock* blocks, size_t n_blocks, size_t scratch_bytes, PwEmpirical** out, uint32_t* status,
                        uint64_t* info);
void pw_empirical_destroy(PwEmpirical* e);
/* Read-outs into caller arrays (a NULL array is skipped). sizes[5] = pcs, ranges (= sum of the pcs' AIR widths), blocks that ran,
 * classes, cells. pcs / counts / air_of_pc: one per pc; range_offsets: pcs + 1; lo_hi: 2 words per range; start_pcs: one per block;
 * class_offsets: blocks + 1 (into the classes); cell_offsets: classes + 1 (into the cells); instruction_column: 2 words per cell. */
void pw_empirical_sizes(const PwEmpirical* e, uint64_t* sizes);
void pw_empirical_read_pcs(const PwEmpirical* e, uint32_t* pcs, uint64_t* counts, uint32_t* air_of_pc, uint64_t* range_offsets);
void pw_empirical_read_ranges(const PwEmpirical* e, uint32_t* lo_hi);
void pw_empirical_read_blocks(const PwEmpirical* e, uint32_t* start_pcs, uint64_t* class_offsets, uint64_t* cell_offsets);
void pw_empirical_read_cells(const PwEmpirical* e, uint32_t* instruction_column);
/* *lo = n / 100, *hi = n * 99 / 100 (the product in more than 64 bits). Host only, no GPU call. */
void pw_empirical_percentile_indices(uint64_t n, uint64_t* lo, uint64_t* hi);
/* A TEST HOOK: ANDed onto both 64-bit fingerprint halves of the calling thread's later pw_empirical_detect calls (0 = the full
 * width), so that a test can make collisions happen. The result stays exact or the status is 6. */
void pw_empirical_set_fingerprint_mask(uint64_t mask);
/* Of the calling thread's last pw_empirical_detect, out[6]: column panels walked, seeds tried, active rows, cells verified, the most
 * scratch bytes held at once, scratch bytes held now. */
void pw_empirical_last_stats(uint64_t* out);

/* ---- superblock detection: basic-block runs, window counts and pc counts of an execution -------------------------
 * What the reference's `detect_superblocks` / `pc_count` (autoprecompiles/src/blocks/mod.rs, execution_profile.rs) compute from the
 * pc trace of an execution, and the body of `count_and_update_execution` (pgo/cell/selection.rs) on a copy that stays on the device.
 * Input: the N pcs in execution order (pw_execution_blocks_from_pcs: a device array, read on the calling thread's launch stream) or
 * the instruction AIRs' traces exactly as pw_empirical_detect takes them (pw_execution_blocks_from_traces: the same bridge
 * evaluation and time order, one copy of the code). `blocks` as for pw_empirical_detect; it must list EVERY block that runs,
 * one-instruction blocks included. max_bb in 1 .. 255 = the reference's superblock_max_bb_count.
 * Heads: position 0 is a head; a head at p of block (s, n) requires pc[p + k] = s + k pc_step for every k < n with p + k < N, and
 * the next head is p + n (a last block cut off by the end of the list counts). Heads of one-instruction blocks cut the head
 * sequence; the maximal stretches of multi-instruction heads between cuts are the runs.
 * Result (host side; sequences of start pcs in lexicographic order, a prefix before its extensions — a BTreeMap<Vec<u64>, _>):
 *   pc counts    per executed pc its number of occurrences, ascending;
 *   runs         the distinct runs, each with the number of times it occurs;
 *   superblocks  for every L in 1 .. max_bb every sequence of L start pcs that occurs as a window inside some run, with the sum over
 *                ALL run instances of the leftmost-greedy non-overlapping occurrences (on a match advance by L, otherwise by 1:
 *                [1,2,1] occurs once in [1,2,1,2,1]). Counts are 64-bit: the reference's u32 wrap is not reproduced.
 * Equal runs are found by 128-bit fingerprints and then VERIFIED element by element against the first run of their group; on a
 * mismatch the grouping is repeated under another seed, three in all. Windows are named exactly, level by level, by sorting.
 * The contract of pw_empirical_detect: the call synchronises before it returns; scratch is per thread, bounded by scratch_bytes
 * (0: half of what the device budget allows) and released on every path; the handle keeps 8 bytes per multi-instruction head on the
 * device. -1 before any GPU call: a NULL pointer, pc_step == 0, a malformed block table, max_bb 0 or above 255, n >= 2^32 (2^32
 * rows), and for the trace route what pw_empirical_detect refuses. An empty execution gives an empty result, status 0.
 * *status: 0 = *out is set (pw_execution_blocks_destroy frees it); 2 = the bound is too small, *info = bytes needed (before an
 * element is read: an upper bound that always suffices); 3 = not block-structured: a head pc that is no start_pc or an in-block pc
 * that does not follow, *info = the smallest offending position (the reference panics on the first and mis-walks on the second) —
 * on the trace route the time key of that row; 4 and 7 as for pw_empirical_detect (trace route); 6 = fingerprint collisions under
 * every seed. Checked in the order 2, 7, 4, 3, 2, 6. With a non-zero status no result exists and 0 is returned. */
typedef struct PwExecutionBlocks PwExecutionBlocks;
int pw_execution_blocks_from_pcs(const uint32_t* d_pcs, uint64_t n, uint32_t pc_step, const PwBasicBlock* blocks, size_t n_blocks,
                                 uint32_t max_bb, size_t scratch_bytes, PwExecutionBlocks** out, uint32_t* status, uint64_t* info);
int pw_execution_blocks_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus,
                                    uint32_t pc_step, const PwBasicBlock* blocks, size_t n_blocks, uint32_t max_bb,
                                    size_t scratch_bytes, PwExecutionBlocks** out, uint32_t* status, uint64_t* info);
void pw_execution_blocks_destroy(PwExecutionBlocks* e);
/* Read-outs into caller arrays (a NULL array is skipped). sizes[6] = pcs, distinct runs, start pcs of all runs, superblocks, start
 * pcs of all superblocks, multi-instruction heads kept on the device. offsets: runs + 1 / superblocks + 1 (into the start pcs). */
void pw_execution_blocks_sizes(const PwExecutionBlocks* e, uint64_t* sizes);
void pw_execution_blocks_read_pc_counts(const PwExecutionBlocks* e, uint32_t* pcs, uint64_t* counts);
void pw_execution_blocks_read_runs(const PwExecutionBlocks* e, uint64_t* offsets, uint32_t* start_pcs, uint64_t* counts);
void pw_execution_blocks_read_superblocks(const PwExecutionBlocks* e, uint64_t* offsets, uint32_t* start_pcs, uint64_t* counts);
/* *count = the leftmost-greedy non-overlapping occurrences of the needle (len start pcs, host memory) over the runs the handle
 * holds now. remove != 0: the counted windows are taken out and what is left of each run becomes separate runs — no later window
 * crosses a removed stretch. A needle with an unknown pc, or longer than every run, gives 0. -1: a NULL pointer or len == 0. */
int pw_execution_blocks_count(PwExecutionBlocks* e, const uint32_t* needle_start_pcs, uint32_t len, int remove, uint64_t* count);
/* A TEST HOOK, as pw_empirical_set_fingerprint_mask: ANDed onto both fingerprint halves of the calling thread's later calls. */
void pw_execution_blocks_set_fingerprint_mask(uint64_t mask);
/* Of the calling thread's last pw_execution_blocks_from_*, out[7]: levels run, clusters counted by pointer doubling, seeds tried,
 * heads, runs, the most scratch bytes held at once (the handle's included), scratch bytes held now. */
void pw_execution_blocks_last_stats(uint64_t* out);

/* ---- selecting APC calls: optimistic constraints and overlapping candidates ----------------------------------------
 * What the reference's `ApcCandidates` (autoprecompiles/src/execution/candidates.rs, with the evaluator of execution/evaluator.rs)
 * decides while an execution runs, computed from the whole execution at once.
 * The execution is n_states = N + 1 states: state i is the machine before instruction i, state N the machine after the last one;
 * the clock of state i is i. d_pcs[i] is its pc, d_regs[r * n_states + i] register r (n_regs >= 0 registers of 32 bits; device
 * arrays, read on the calling thread's launch stream). limb_bits in 1 .. 32.
 * APC a (host array, any order, apc_id = the index) starts at start_pc, spans cycle_count >= 1 instructions and owns the constraints
 * [first_constraint, first_constraint + n_constraints) of the flat host array. A constraint says left == right; an operand is
 * kind 0 Number(value), kind 1 Pc(instr_idx) = the pc of state s + instr_idx, or kind 2 RegisterLimb(instr_idx, reg, limb) =
 * (register reg of state s + instr_idx >> limb * limb_bits) & (2^limb_bits - 1), s being the candidate's first state. A constraint's
 * step is the largest instr_idx among its literals, 0 without one.
 * Semantics: for i = 0 .. N: check_conditions(state i); extract_calls(); try_insert(state i, a) for every APC with start_pc ==
 * d_pcs[i], in ascending apc_id. After state N: abort_in_progress(), extract_calls(). So a candidate (a, s) is inserted iff every
 * constraint of step 0 holds, fails at the first step k <= cycle_count with a false constraint (a constraint of a larger step is
 * never checked), is done at state s + cycle_count with the range [s, s + cycle_count), and is aborted if s + cycle_count > N.
 * extract_calls folds the done candidates in insertion order over all pairs (i < j): if neither is discarded and the ranges overlap,
 * the lower rank is discarded, rank = (priority, length, earlier insertion). The fold is order-dependent — a candidate discards
 * lower-ranked followers until it meets a higher-ranked one, and what it discarded stays discarded — and is reproduced exactly.
 * Result (host side): the calls (apc_id, from, to) in insertion order; per APC seven 64-bit counters: pc matches, refused at
 * insertion, failed later, aborted at the end, done, discarded by the fold, calls (matches = refused + failed + aborted + done,
 * done = discarded + calls); the number of positions covered by calls.
 * pw_apc_calls_from_traces takes the instruction AIRs' traces exactly as pw_execution_blocks_from_traces takes them (the same bridge
 * evaluation and time order): the states are the pcs of the active rows in time order and final_pc, the pc after the last row (the
 * bridge's receive does not carry it). Pcs only: there are no registers, so a RegisterLimb operand is refused. segment_of_air must
 * name ONE segment (NULL = 0): the reference aborts candidates at a segment's end, so segments are selected one by one. The result
 * also holds the time key (segment << 32 | timestamp) of every position.
 * The contract of pw_empirical_detect: the call synchronises before it returns; scratch is per thread, bounded by scratch_bytes
 * (0: half of what the device budget allows) and released on every path; the APC table and the constraints are copied to the device
 * once per call. -1 before any GPU call: a NULL pointer, cycle_count == 0, a constraint span outside the array, an operand kind
 * above 2, reg >= n_regs, limb_bits outside 1 .. 32, limb * limb_bits >= 32, n_states >= 2^32 or n_states times the largest number
 * of APCs sharing a start pc >= 2^32, two segment numbers on the trace route, and there what pw_empirical_detect refuses.
 * n_states == 0 gives an empty result, status 0.
 * *status: 0 = *out is set (pw_apc_calls_destroy frees it); 2 = the bound is too small, *info = bytes that always suffice (decided
 * before an element is read); 4 and 7 as for pw_empirical_detect (trace route). Checked in the order 2, 7, 4. With a non-zero
 * status no result exists and 0 is returned. */
typedef struct { uint32_t kind, instr_idx, reg, limb; uint64_t value; } PwApcOperand;
typedef struct { PwApcOperand left, right; } PwApcConstraint;
typedef struct { uint32_t start_pc, cycle_count; uint64_t priority, first_constraint, n_constraints; } PwApc;
typedef struct PwApcCalls PwApcCalls;
int pw_apc_calls_from_states(const uint32_t* d_pcs, const uint32_t* d_regs, uint64_t n_states, uint32_t n_regs, uint32_t limb_bits,
                             const PwApc* apcs, size_t n_apcs, const PwApcConstraint* constraints, size_t n_constraints,
                             size_t scratch_bytes, PwApcCalls** out, uint32_t* status, uint64_t* info);
int pw_apc_calls_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bus, uint32_t final_pc,
                             const PwApc* apcs, size_t n_apcs, const PwApcConstraint* constraints, size_t n_constraints,
                             size_t scratch_bytes, PwApcCalls** out, uint32_t* status, uint64_t* info);
void pw_apc_calls_destroy(PwApcCalls* e);
/* Read-outs into caller arrays (a NULL array is skipped). sizes[5] = calls, APCs, positions covered by calls, states, time keys
 * (trace route: N, otherwise 0). apc_ids / from / to: one per call; counters: 7 per APC in the order above; keys: one per position. */
void pw_apc_calls_sizes(const PwApcCalls* e, uint64_t* sizes);
void pw_apc_calls_read_calls(const PwApcCalls* e, uint32_t* apc_ids, uint64_t* from, uint64_t* to);
void pw_apc_calls_read_counters(const PwApcCalls* e, uint64_t* counters);
void pw_apc_calls_read_time_keys(const PwApcCalls* e, uint64_t* keys);
/* A TEST HOOK, in the style of pw_execution_blocks_set_fingerprint_mask: components of more than n candidates take the long path
 * of the fold in the calling thread's later calls (0 = the default, 32), so that small inputs reach it. The result does not change. */
void pw_apc_calls_set_long_threshold(uint64_t n);
/* Of the calling thread's last pw_apc_calls_from_*, out[7]: candidates, valid (done) candidates, components, the longest component,
 * components on the long path, the most scratch bytes held at once, scratch bytes held now. */
void pw_apc_calls_last_stats(uint64_t* out);

/* ---- the states of an execution from its traces: pcs, registers, time keys -----------------------------------------
 * What pw_apc_calls_from_states wants, built where the traces lie. Positions, time keys and pcs are those of
 * pw_apc_calls_from_traces (bridge_bus = its bus): state i < N is the machine before the active row with the i-th smallest
 * timestamp ts_i, state N the machine after the last row with pc final_pc. The registers are read off the memory bus: a register
 * access is an active interaction on memory_bus (as, ptr, d0, d1, d2, d3, t) with as == reg_as; its register is ptr / reg_ptr_step
 * (4 for RV32), its word d0 | d1 << 8 | d2 << 16 | d3 << 24. Interactions in other address spaces are skipped, and so are
 * accesses to registers nobody asked for, once ptr is evaluated. A send (+1) with timestamp t is seen from state
 * p = #{ j < N : ts_j <= t } on (it belongs to instruction p - 1, so 1 <= p <= N); of several sends to one register with one p the
 * largest t wins. A receive (-1) carries (previous word, previous timestamp): per register the receive with the smallest previous
 * timestamp holds the register's value at state 0. The value of a register at state i is the word of the last send with p <= i, or
 * the value at state 0 without one. initial_regs (optional) is the machine at the segment's start: with it a register that is never
 * received has that word at state 0, and a first receive that disagrees is status 10; without it a requested register that is
 * never received is status 9. Whether every receive finds what the previous send left is pw_check_segment_buses' business, not
 * this routine's. Only original-instruction AIRs are meant: one instruction per active row.
 * pw_execution_states_from_traces: regs = n_regs distinct register numbers (host), row k of the table is register regs[k];
 * initial_regs NULL or n_regs host words, one per row. The handle owns three device arrays: pcs[N + 1], regs[n_regs x (N + 1)]
 * (row k at k * (N + 1): the layout pw_apc_calls_from_states reads) and the N time keys.
 * pw_apc_calls_from_traces_registers: pw_apc_calls_from_traces with RegisterLimb operands. n_regs bounds the reg of a literal, as
 * on the states route; initial_regs NULL or n_regs host words indexed by register. Only the distinct registers the constraints
 * name become rows; the table never leaves the device. The result carries the time keys; without a register literal it equals
 * pw_apc_calls_from_traces'.
 * The contract of pw_apc_calls_from_traces: the call synchronises before it returns; scratch is per thread, bounded by scratch_bytes
 * (0: half of what the device budget allows; the handle's own arrays count) and released on every path; one segment number per
 * call. -1 before any GPU call: a NULL pointer, reg_ptr_step == 0, an entry of regs twice or with regs[k] * reg_ptr_step >= p, more
 * than 65535 rows, a bus id >= p, two segment numbers, an interaction on memory_bus with an arity other than 7, and whatever
 * pw_apc_calls_from_traces refuses.
 * *status: 0 = *out is set; 2 = the bound is too small, *info = bytes that always suffice (decided before an element is read); 7
 * and 4 as for pw_apc_calls_from_traces; 8 = a register tuple that is none, *info = the smallest packed witness
 * (air << 46 | interaction << 26 | row) among: a multiplicity other than +-1, ptr no multiple of the step, a data word >= 256, two
 * sends with one (register, timestamp), a send before ts_0; 9 = a requested register without a value, *info = the smallest such
 * register; 10 = initial_regs contradicted by the first receive, *info = the smallest such register. Checked in the order 2, 7, 4,
 * 8, 9, 10. With a non-zero status no result exists and 0 is returned. */
typedef struct PwExecutionStates PwExecutionStates;
int pw_execution_states_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                                    uint32_t memory_bus, uint32_t final_pc, uint32_t reg_as, uint32_t reg_ptr_step, const uint32_t* regs,
                                    size_t n_regs, const uint32_t* initial_regs, size_t scratch_bytes, PwExecutionStates** out,
                                    uint32_t* status, uint64_t* info);
void pw_execution_states_destroy(PwExecutionStates* e);
/* sizes[4] = states (N + 1), registers (rows), register sends read, device bytes the handle holds. */
void pw_execution_states_sizes(const PwExecutionStates* e, uint64_t* sizes);
/* The handle's device arrays (a NULL argument is skipped); they live until pw_execution_states_destroy. */
void pw_execution_states_device(const PwExecutionStates* e, const uint32_t** d_pcs, const uint32_t** d_regs, const uint64_t** d_time_keys);
/* Copies into host arrays of N + 1, n_regs x (N + 1) and N elements (a NULL array is skipped). -1: a NULL handle. */
int pw_execution_states_read(const PwExecutionStates* e, uint32_t* pcs, uint32_t* regs, uint64_t* time_keys);
/* Of the calling thread's last pw_execution_states_from_traces, out[5]: register sends read, sends kept after placing, the table
 * words a workgroup of the fill writes (its tile), the most scratch bytes held at once (the handle's included), scratch bytes held
 * now. */
void pw_execution_states_last_stats(uint64_t* out);
int pw_apc_calls_from_traces_registers(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                                       uint32_t memory_bus, uint32_t final_pc, uint32_t reg_as, uint32_t reg_ptr_step, uint32_t n_regs,
                                       uint32_t limb_bits, const uint32_t* initial_regs, const PwApc* apcs, size_t n_apcs,
                                       const PwApcConstraint* constraints, size_t n_constraints, size_t scratch_bytes, PwApcCalls** out,
                                       uint32_t* status, uint64_t* info);

/* ---- applying APC calls: per-APC source traces and residual chip traces -------------------------------------------
 * pw_trace_gather_rows: the row gather on caller-owned device buffers, all jobs in ONE launch. Per job (a host record holding device
 * pointers) out[c * h_out + i] = idx[i] < h_in ? in[c * h_in + idx[i]] : 0 for c < width, i < h_out: `in` is a column-major
 * width x h_in matrix, `out` a column-major width x h_out matrix of which EVERY word is written, idx h_out row numbers; 0xFFFFFFFF
 * means "zero row" (and so does any other index that is no row of `in`). Words are copied bit for bit. A lane owns 4 consecutive
 * output rows and stores 16 bytes at once; 4 consecutive source rows at a 16-byte aligned address are one 16-byte load. h_out < 4, or
 * an `out` / `idx` that is not 16-byte aligned, takes a word-by-word path. -1 before any GPU call: a NULL pointer in a job (or jobs
 * NULL with n_jobs > 0), h_in or h_out no power of two, h_in > 2^31, h_out > 2^32, width == 0 or >= 2^32. The outputs of two jobs
 * must not overlap. The call runs on the calling thread's launch stream and synchronises before it returns.
 *
 * pw_apc_sources_from_traces: positions, time keys and the map position -> (AIR, row) are pw_apc_calls_from_traces' (bridge_bus =
 * its bus): position i < N is the active row with the i-th smallest time key. One instruction per active row: original-instruction
 * AIRs only. An AIR without a two-argument interaction on bridge_bus takes no part and gets no output. APC a spans
 * cycle_counts[a] >= 1 instructions; the calls are three host arrays (apc_id, from, to), strictly ascending in from, non-overlapping,
 * to - from == cycle_counts[apc_id]: what pw_apc_calls_read_calls returns.
 * Sources: for APC a with calls c_0 .. c_(n-1) in start order, air_a[k] = the AIR of position from_0 + k (the same for every call, or
 * status 12), occ_a[k] = #{k' < k : air_a[k'] == air_a[k]}, rbs_a[A] = #{k : air_a[k] == A}. For every AIR A with rbs_a[A] > 0 the
 * source matrix S is column-major, of A's width and height H = max(2^min_log_height, next power of two >= n * rbs_a[A]), with
 * S[c * H + j * rbs + occ_a[k]] = trace_A[c * H_A + row(from_j + k)] for every k with air_a[k] == A and every other row zero: the
 * OriginalAir {width, H, S, rbs} of include/powdr_gpu.h with Subst.row = occ_a[k].
 * Residuals: for every AIR A that takes part, the active rows of A at no covered position in ascending row order, in a matrix of
 * height max(2^min_log_height, next power of two >= their number) whose other rows are zero — the padding convention of
 * powdr_original_airs_expand. An AIR whose idle row is not the zero row is outside this contract.
 * Nothing in either output depends on an order of arrival. The handle owns the matrices; the originals are left as they are.
 * The contract of pw_apc_calls_from_traces: the call synchronises before it returns; scratch is per thread, bounded by scratch_bytes
 * (0: half of what the device budget allows; the handle's own matrices count) and released on every path; one segment number per
 * call. -1 before any GPU call: a NULL pointer, apc_id >= n_apcs, cycle_count == 0, to - from != cycle_count, calls unsorted or
 * overlapping, min_log_height > 31, two segment numbers, and whatever pw_apc_calls_from_traces refuses about the AIR list.
 * *status: 0 = *out is set (pw_apc_sources_destroy frees it; the matrices live until then); 2 = the bound is too small, *info =
 * bytes that always suffice (decided before an element is read); 7 and 4 as for pw_apc_calls_from_traces; 11 = a call with to > N,
 * *info = the smallest such call index; 12 = two calls of one APC disagree on the AIR of an instruction, *info = the smallest
 * position that disagrees with the APC's first call. Checked in the order 2, 7, 4, 11, 12. With a non-zero status no result exists
 * and 0 is returned. */
typedef struct PwGatherJob {
    const uint32_t* in; /* device, column-major width x h_in */
    uint64_t h_in;
    uint64_t width;
    const uint32_t* idx; /* device, h_out row numbers of `in`, 0xFFFFFFFF = zero row */
    uint32_t* out;       /* device, column-major width x h_out */
    uint64_t h_out;
} PwGatherJob;
int pw_trace_gather_rows(const PwGatherJob* jobs, size_t n_jobs);
typedef struct PwApcSources PwApcSources;
int pw_apc_sources_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                               const uint32_t* cycle_counts, size_t n_apcs, const uint32_t* call_apc_ids, const uint64_t* call_from,
                               const uint64_t* call_to, size_t n_calls, uint32_t min_log_height, size_t scratch_bytes, PwApcSources** out,
                               uint32_t* status, uint64_t* info);
void pw_apc_sources_destroy(PwApcSources* e);
/* sizes[6] = APCs, AIRs, positions (N), covered positions, bytes of the source matrices, bytes of the residual matrices. */
void pw_apc_sources_sizes(const PwApcSources* e, uint64_t* sizes);
/* The layout of APC apc: *n_calls, and for an APC with calls air[k], occ[k] of its cycle_count instructions (NULL arguments are
 * skipped). Returns the number of entries written per array (0 for an APC without calls: its layout is unknown), -1 for a NULL
 * handle or apc >= n_apcs. */
int64_t pw_apc_sources_layout(const PwApcSources* e, uint32_t apc, uint64_t* n_calls, uint32_t* air, uint32_t* occ);
/* The source matrix of (apc, air): device pointer, width, height, row_block_size — height 0 (and a NULL pointer) where the APC does
 * not use the AIR. -1: a NULL handle, apc >= n_apcs, air >= n_airs. */
int pw_apc_sources_source(const PwApcSources* e, uint32_t apc, uint32_t air, const uint32_t** d_matrix, uint32_t* width, uint64_t* height,
                          uint32_t* row_block_size);
/* The residual of AIR air: device pointer, rows kept, log_height. Returns 1, 0 for an AIR that takes no part (no matrix), -1 for a
 * NULL handle or air >= n_airs. */
int pw_apc_sources_residual(const PwApcSources* e, uint32_t air, const uint32_t** d_matrix, uint64_t* rows, uint32_t* log_height);
/* Copies of a whole matrix into a host array of width x height words (nothing is written where there is no matrix). -1: a NULL
 * argument or an index out of range. */
int pw_apc_sources_read_source(const PwApcSources* e, uint32_t apc, uint32_t air, uint32_t* words);
int pw_apc_sources_read_residual(const PwApcSources* e, uint32_t air, uint32_t* words);
/* Of the calling thread's last pw_apc_sources_from_traces or pw_trace_gather_rows, out[8]: covered positions, source bytes, residual
 * bytes, gather jobs, gather tiles (1 024 rows x 16 columns) whose loads were all 16-byte loads, tiles with 4-byte loads, the most
 * scratch bytes held at once (the handle's matrices included), scratch bytes held now. */
void pw_apc_sources_last_stats(uint64_t* out);

/* ---- applying APC calls, direct mode: APC traces straight from the chips' traces ----------------------------------
 * pw_apc_sources_from_traces_flags: flags == 0 is pw_apc_sources_from_traces, the same results and statuses. PW_APC_SOURCES_DIRECT
 * builds NO source matrices: the handle keeps, in one device allocation of its own, the index lists the place stage makes — for every
 * (APC a, AIR A) with rbs_a[A] > 0 the list L of n * rbs words with L[j * rbs + occ_a[k]] = row(from_j + k) for every k with
 * air_a[k] == A — and remembers each participating AIR's trace pointer, height and width: THE CALLER'S TRACES MUST STAY ALIVE AND
 * UNCHANGED UNTIL THE LAST pw_apc_sources_tracegen ON THE HANDLE. Layout, residuals, the statuses 7, 4, 11, 12 and their order are
 * those of flags 0; the bound of status 2 counts the lists where flags 0 counts the source matrices. On a direct handle
 * pw_apc_sources_source reports height 0 and a NULL pointer for every pair (width and row_block_size as with flags 0),
 * pw_apc_sources_read_source writes nothing and sizes[4] is 0. Any other bit of flags: -1.
 * pw_apc_sources_index_bytes: the bytes of the handle's index lists, 0 on a flags-0 handle (and for a NULL handle).
 *
 * pw_apc_sources_tracegen: for every job, every cell {instr, col, apc_col} of it and every r < out_height, with (A, occ) the layout
 * entry of instr in APC job.apc, L that pair's list and H_A the height of A's trace:
 *   d_out[apc_col * out_height + r] = r < n_calls(apc) ? trace_A[col * H_A + L[r * rbs + occ]] : 0
 * — word for word what _apc_tracegen writes from the source matrices of flags 0 with Subst {A, col, occ, apc_col}. d_out is a
 * column-major out_width x out_height matrix on the device; columns no cell names are NOT touched (derived columns are written
 * later, by _apc_apply_derived_expr); one source cell may feed several APC columns; the cells are host arrays in any order. A job
 * for an APC without calls writes zeros into the columns it names. ALL jobs of a call are ONE launch: a workgroup is (job,
 * instruction, tile of 1 024 rows, group of up to 16 of the instruction's cells); a lane owns 4 consecutive rows, reads its 4 list
 * entries once and stores 16 bytes per cell; 4 consecutive source rows at a 16-byte aligned address are one 16-byte load.
 * out_height < 4, or a d_out off the 16-byte grid, goes word by word. A list entry that is no row of the AIR reads as zero.
 * -1 before any GPU call: a NULL argument (the handle; jobs with n_jobs > 0; cells with n_cells > 0; d_out), a handle that is not
 * direct, apc >= n_apcs, instr >= the APC's cycle count, col >= the AIR's width (for an APC with calls: without calls its AIRs are
 * unknown), apc_col >= out_width, two cells of a job with one apc_col, out_height no power of two or > 2^32 or < n_calls(apc),
 * out_width == 0, two jobs whose output matrices overlap. The call runs on the calling thread's launch stream and synchronises
 * before it returns; its tables go through the per-thread scratch of pw_apc_sources_from_traces and are released on every path.
 * pw_apc_sources_tracegen_last_stats: of the calling thread's last pw_apc_sources_tracegen, out[6]: jobs, work items (job,
 * instruction, cell group), tiles whose loads were all 16-byte loads (or none: zero rows), tiles with 4-byte loads, bytes
 * written, scratch bytes held now. */
#define PW_APC_SOURCES_DIRECT 1u
typedef struct PwApcCell {
    uint32_t instr;   /* instruction of the APC: < its cycle count */
    uint32_t col;     /* column of that instruction's AIR */
    uint32_t apc_col; /* column of d_out */
} PwApcCell;
typedef struct PwApcTraceJob {
    uint32_t apc;
    const PwApcCell* cells; /* host */
    size_t n_cells;
    uint32_t* d_out; /* device, column-major out_width x out_height */
    uint64_t out_height;
    uint32_t out_width;
} PwApcTraceJob;
int pw_apc_sources_from_traces_flags(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                                     const uint32_t* cycle_counts, size_t n_apcs, const uint32_t* call_apc_ids,
                                     const uint64_t* call_from, const uint64_t* call_to, size_t n_calls, uint32_t min_log_height,
                                     size_t scratch_bytes, uint32_t flags, PwApcSources** out, uint32_t* status, uint64_t* info);
uint64_t pw_apc_sources_index_bytes(const PwApcSources* e);
int pw_apc_sources_tracegen(const PwApcSources* e, const PwApcTraceJob* jobs, size_t n_jobs);
void pw_apc_sources_tracegen_last_stats(uint64_t* out);

/* ---- cutting an execution into segments under APC-aware limits ----------------------------------------------------
 * pw_execution_segments_from_traces: positions 0 .. N, their time keys and the map position -> (AIR, row) are exactly
 * pw_apc_sources_from_traces' (the same bridge evaluation and time sort): original-instruction AIRs only, one instruction per active
 * row, an AIR without a two-argument interaction on bridge_bus takes no part, one segment number for all AIRs. The calls (n_calls may
 * be 0) are three host arrays as pw_apc_calls_read_calls returns them: strictly ascending in from, non-overlapping,
 * to - from == cycle_counts[apc_id].
 * Classes: there are n_airs + n_apcs. A position covered by call j has class n_airs + apc_id(j) if it is from_j and no class
 * otherwise; an uncovered position has the class of its AIR. cnt_c(p, q) = the positions of class c in [p, q); width_c = the prover's
 * width of an AIR class, apc_widths[a] of an APC class. padded(n) = 0 for n == 0, else max(2^min_log_height, next power of two >= n).
 * fits(p, q): every cnt_c(p, q) <= 2^max_log_height, and max_cells == 0 or sum_c width_c * padded(cnt_c(p, q)) <= max_cells (the sum
 * is compared as the integer it is: the device adds with saturation at 2^64 - 1). allowed(q): no call has from < q < to.
 * Cuts: b_0 = 0; b_(s+1) = the largest allowed q in (b_s, N] with fits(b_s, q); until b_S == N. fits is monotone in q, so no valid
 * cut has fewer segments. N == 0 gives S == 0. This definition is this project's own (the reference's metering code is not part of
 * its checkout); it meters the ACCELERATED program: a call counts as one row of its APC and is never cut.
 * Results (host side): S; b[0 .. S]; per segment the time key and pc of its first position, pc[S] = final_pc; first_call[0 .. S]: the
 * calls of segment s are first_call[s] .. first_call[s + 1]; cnt_c(b_s, b_(s+1)) for every class. On the device, for every (segment,
 * participating AIR A with a position in it) a row list: the rows of A at the positions of [b_s, b_(s+1)), COVERED ONES INCLUDED, in
 * ascending position, padded with 0xFFFFFFFF to padded(rows), 16-byte aligned: what PwGatherJob.idx takes. The handle keeps the
 * lists (4 bytes per entry) and no matrices; the caller gathers a segment into buffers of its own. With calls the ORIGINAL trace of a
 * segment may be taller than the cap: the cap binds the residuals and the APC traces, which is what gets proven. System AIRs
 * (boundary, Merkle, program, connector) are not metered.
 * The contract of pw_apc_sources_from_traces: the call runs on the calling thread's launch stream and synchronises before it returns;
 * scratch is per thread, bounded by scratch_bytes (0: half of what the device budget allows; the handle's lists count) and
 * everything but the lists is released on every path. Results are identical on every run.
 * -1 before any GPU call: whatever pw_apc_sources_from_traces refuses about the AIRs and the calls, a NULL limits pointer,
 * max_log_height > 31, min_log_height > max_log_height, apc_widths == NULL with n_apcs > 0 and max_cells > 0, a zero apc_widths[a]
 * under max_cells > 0.
 * *status: 0 = *out is set (pw_execution_segments_destroy frees it); 2 = the bound is too small, *info = bytes that always suffice
 * (decided before an element is read); 7 and 4 as for pw_apc_calls_from_traces; 11 = a call with to > N, *info = the smallest such
 * call index; 13 = nothing fits: no allowed q > b_s satisfies fits(b_s, q) (only possible under max_cells), *info = b_s; 14 = more
 * than max_segments segments (0 means 2^20), *info = the position reached. Checked in the order 2, 7, 4, 11, 13, 14 (13 and 14 in
 * the order the cuts meet them). With a non-zero status no result exists and 0 is returned. */
typedef struct { uint32_t max_log_height, min_log_height; uint64_t max_cells, max_segments; } PwSegmentLimits;
typedef struct PwExecutionSegments PwExecutionSegments;
int pw_execution_segments_from_traces(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                                      uint32_t final_pc, const uint32_t* cycle_counts, const uint32_t* apc_widths, size_t n_apcs,
                                      const uint32_t* call_apc_ids, const uint64_t* call_from, const uint64_t* call_to, size_t n_calls,
                                      const PwSegmentLimits* limits, size_t scratch_bytes, PwExecutionSegments** out, uint32_t* status,
                                      uint64_t* info);
void pw_execution_segments_destroy(PwExecutionSegments* e);
/* sizes[6] = segments (S), AIRs, APCs, positions (N), covered positions, bytes of the row lists. */
void pw_execution_segments_sizes(const PwExecutionSegments* e, uint64_t* sizes);
/* Read-outs into caller arrays (a NULL array is skipped): positions[S + 1] = b, time_keys[S], pcs[S + 1], first_call[S + 1]. */
void pw_execution_segments_read_bounds(const PwExecutionSegments* e, uint64_t* positions, uint64_t* time_keys, uint32_t* pcs,
                                       uint64_t* first_call);
/* rows[s * (n_airs + n_apcs) + c] = cnt_c(b_s, b_(s+1)): class c < n_airs is AIR c (0 for an AIR that takes no part), class
 * n_airs + a is APC a. */
void pw_execution_segments_read_heights(const PwExecutionSegments* e, uint64_t* rows);
/* The row list of (segment, air): device pointer, its rows and log2 of its padded length. Returns 1, 0 where the AIR has no row in
 * the segment (no list: NULL, 0, 0), -1 for a NULL handle, segment >= S or air >= n_airs. The list lives until
 * pw_execution_segments_destroy. */
int pw_execution_segments_rows(const PwExecutionSegments* e, uint32_t segment, uint32_t air, const uint32_t** d_idx, uint64_t* rows,
                               uint32_t* log_height);
/* All row lists at once, for tests and tools: the lists lie in ONE device allocation of sizes[5] bytes, in (segment, AIR) order;
 * *d_base = its first word (NULL without lists), so that the list of (segment, air) begins at word d_idx - *d_base; words (NULL:
 * skipped) receives a copy of the whole allocation. -1: a NULL handle. */
int pw_execution_segments_read_lists(const PwExecutionSegments* e, uint32_t* words, const uint32_t** d_base);
/* Of the calling thread's last pw_execution_segments_from_traces, out[6]: segments, classes, cell-bound probes (workgroup sums of the
 * bisection), cuts snapped to a call's start, the most scratch bytes held at once (the handle's lists included), scratch bytes held
 * now. */
void pw_execution_segments_last_stats(uint64_t* out);

/* ---- the same cut with the system AIRs' heights metered -----------------------------------------------------------
 * pw_execution_segments_from_traces_metered: everything above, and per candidate segment the heights of the memory boundary AIR, the
 * memory Merkle AIR and the Poseidon2 chip that close_segment will give it, as further limits of the cut.
 * Access: an active interaction (non-zero multiplicity, either sign) on meter->memory_bus of the row at a position; the row's AIR
 * takes part in the bridge; the interaction has the 7 arguments (as, ptr, d0..d3, t). Its key is (as - 1) * 2^29 + ptr, the key of
 * pw_memory_tree_boundary_leaves; data words and timestamps are not read; covered positions count like uncovered ones.
 * For a window [p, q): B(p, q) = the distinct keys of the accesses at its positions; M(p, q) = the distinct pairs (l, key >> l),
 * l = 0 .. tree_height, over those keys (the nodes of the union of their root paths: pw_memory_merkle_trace's n_nodes);
 * P(p, q) = 2 * M(p, q), an UPPER BOUND on the Poseidon2 chip's rows, not a count: the chip dedupes by input words.
 * fits_sys(p, q): fits(p, q), B <= 2^max_log_height[0], M <= 2^max_log_height[1], P <= 2^max_log_height[2], and under max_cells > 0
 * the cell sum gains width[k] * padded_sys(count_k) for every k with width[k] > 0 (still saturating), padded_sys(0) = 0, else
 * padded_sys(n) = max(2, padded(n)). The cuts are the greedy cuts under fits_sys. The largest q that fits may now lie strictly
 * inside a call (a covered position can touch a new block): it moves down to the call's start, last_stats' fourth word counts it,
 * and a moved cut that lands on b_s is status 13, which can therefore occur without max_cells.
 * -1 before any GPU call, besides the above: a NULL meter, memory_bus >= p, tree_height outside 1 .. 30, a max_log_height[k] > 31,
 * an interaction on memory_bus with another arity than 7.
 * *status 15 = an access without a key: as not 1 or 2, ptr >= 2^29 or key >= 2^tree_height; *info = the smallest packed witness
 * (air << 46 | interaction << 26 | row). Checked in the order 2, 7, 4, 11, 15, 13 / 14.
 * pw_execution_segments_from_traces itself is unchanged; a handle from it answers pw_execution_segments_read_system_heights with
 * zeros. */
typedef struct { uint32_t memory_bus, tree_height, max_log_height[3], width[3]; } PwSystemMeter; /* 0 boundary, 1 Merkle, 2 Poseidon2 */
int pw_execution_segments_from_traces_metered(const PwSegmentAir* airs, const uint32_t* segment_of_air, size_t n_airs, uint32_t bridge_bus,
                                              uint32_t final_pc, const uint32_t* cycle_counts, const uint32_t* apc_widths, size_t n_apcs,
                                              const uint32_t* call_apc_ids, const uint64_t* call_from, const uint64_t* call_to,
                                              size_t n_calls, const PwSegmentLimits* limits, const PwSystemMeter* meter,
                                              size_t scratch_bytes, PwExecutionSegments** out, uint32_t* status, uint64_t* info);
/* rows[s * 3 + k] = B, M, 2 M of segment s. */
void pw_execution_segments_read_system_heights(const PwExecutionSegments* e, uint64_t* rows);
/* Of the calling thread's last metered cut, out[6]: accesses walked, tiles inserted, the most slots the node table had, nodes
 * inserted past the cuts (the overshoot: at most one tile per segment), host synchronisations of the per-segment loop, node tables
 * cleared (growth restarts included). Zeros after an unmetered cut. */
void pw_execution_segments_last_meter_stats(uint64_t* out);
/* A test knob of the calling thread: the positions of one tile of the meter (0 = the default, 2^14). Results do not depend on it. */
void pw_execution_segments_set_meter_tile(uint64_t n);

/* ---- the sparse memory Merkle tree ---------------------------------------------------------------------------------
 * A binary Poseidon2 tree of `height` H over 2^H leaves of 8 field words, kept on the device from segment to segment: leaf digest =
 * the first 8 words of permute(payload | 0^8), node = the first 8 words of permute(left | right) — the tuple of the compression bus —
 * Z_0 = the digest of the zero payload, Z_(l+1) = compress(Z_l, Z_l): a subtree nobody has written hashes to Z_l and is not stored,
 * an empty tree's root is Z_H. Per level the device holds the sorted indices and digests of the stored nodes (level 0: the payloads
 * too), Montgomery words below p. The memory of §5j is H = 30 with the key (as - 1) * 2^29 + ptr.
 *
 * pw_memory_tree_create: NULL unless 1 <= height <= 40. Z_0 .. Z_H are computed on the host and device memory is allocated by the
 * first call that needs it: creating a tree and asking an empty tree for its root need no GPU. The tree keeps a copy of the round
 * constants installed when it is made (pw_get_poseidon2_constants); EVERY call below compares them with the installed table and
 * returns -1 when they differ — a tree is as tied to its table as the Poseidon2 chip's AIR is.
 * pw_memory_tree_root: out[8] = the root, canonical words on the host (no GPU call).
 * pw_memory_tree_stats: stored leaves; stored nodes over all levels (the leaves included); device bytes held; and of the last
 * pw_memory_tree_update that ended with status 0: permutations hashed, launches (the library's own kernels; a rocPRIM select or scan
 * counts as one), the most scratch bytes held at once (all three zero after an update of n = 0 keys).
 *
 * pw_memory_tree_update: d_keys = n strictly increasing leaf indices below 2^H; d_init, d_fin = 8 words per key, row-major,
 * Montgomery. In this order: (1) validation — *status 4: the keys are not strictly increasing or one is >= 2^H; 5: a payload word
 * >= p; *info = the index of the first offending key; (2) continuity — for every key the stored payload (the zero payload for a leaf
 * that is not stored) must equal its d_init words: *status 3, *info = the smallest mismatching KEY; (3) the record count — the touched
 * node sets are T_0 = the keys, T_l = unique(T_(l-1) >> 1); *n_rows = 2 (n + sum_(l=1..H) |T_l|), *log_height = the smallest height
 * >= 1 that holds them; with d_records != NULL and cap_log_height < *log_height: *status 1 and nothing is written; (4) the phase-0
 * records from the tree as it stands, the new tree (the payloads become d_fin), the phase-1 records from the new tree.
 * d_records (may be NULL: no records) = 25 columns [valid, left[8], right[8], out[8]], column-major with pitch 2^*log_height,
 * Montgomery: valid = 1 on the *n_rows rows, all 25 words zero on the padding rows. Row order: phase (0 = before, 1 = after); inside
 * a phase level 0 in key order, then the nodes of T_1, .., T_H, each by index. A level-0 row is (payload, 0^8, leaf digest), a
 * level-l row (left child digest, right child digest, node digest) with the defaults Z_(l-1), Z_l where a node is not stored; the
 * last row of each phase has the root as `out`. d_node_ids (optional, needs d_records): one uint64 per row, phase << 63 | level <<
 * 56 | index. Every byte is independent of the order of arrival: the keys are sorted and unique and every output place is a rank.
 * LOAD MODE: d_init == NULL skips continuity and records and just writes the payloads (an initial image); d_records and d_node_ids
 * must then be NULL, log_height and n_rows may be.
 * With any non-zero *status or return value the tree is exactly what it was (the new tree is built into fresh buffers and swapped in
 * at the end). Malformed arguments (a NULL where a pointer is required, a tree whose buffers live on another device, changed round
 * constants): -1 before any GPU call. The call runs on the calling thread's launch stream, synchronises before it returns and frees
 * its scratch on every path (the contract of pw_memory_boundary_trace). A leaf written with the zero payload stays stored: its digest
 * is Z_0, the root is the one of a tree without it.
 *
 * pw_memory_tree_set_mode / pw_memory_tree_get_mode: how pw_memory_tree_update makes the levels above level 0. Nothing else depends on
 * the mode: statuses and *info, *n_rows, *log_height, records, node ids, the root and every stored byte are the same in both, a
 * non-zero status or return value leaves the tree as it was, and no byte depends on an order of arrival. The mode may be changed
 * between any two updates of one tree; neither call touches the GPU, both work on a tree without device buffers. -1: a NULL pointer,
 * an unknown mode, changed round constants.
 *   PW_MEMORY_TREE_REBUILD (0, the default): level 0 is merged by ranks and only the update's leaves are hashed; every level above is
 *   hashed again from the level below. last_permutations = n + sum_(l>=1) s_l (s_l = the stored nodes of level l afterwards).
 *   PW_MEMORY_TREE_INCREMENTAL (1): with L = the number of levels l >= 1 whose level l - 1 holds more than 1024 nodes afterwards (the
 *   levels the rebuild gives a launch of their own), the levels 1 .. L are rank merges too: the nodes of T_l are hashed, once each,
 *   from their children in the new level l - 1, and every other stored node moves to its new rank with its index and digest, unhashed.
 *   The levels above L are finished by the one workgroup that finishes them in the rebuild. last_permutations = n + sum_(l=1..L) |T_l|
 *   + sum_(l>L) s_l; last_launches also counts the one read-back each of those L levels needs (the size of the new level), and
 *   last_scratch_bytes the touched sets, which stay until the levels are merged. The new tree is built next to the old one as in the
 *   rebuild (not in place). LOAD MODE is the full rebuild in both modes.
 *
 * pw_memory_tree_boundary_leaves: the leaves of a memory boundary trace (pw_memory_boundary_trace: 18 columns, 2^log_height rows, the
 * first n_locations valid, sorted by (as, ptr), hence by key): d_keys[r] = (as - 1) * 2^29 + ptr, d_init / d_fin[8 r ..] = (init0..3,
 * 0, 0, 0, 0) / (fin0..3, 0, 0, 0, 0). -1: a NULL pointer, log_height outside 1 .. 40, more locations than rows.
 *
 * pw_memory_tree_open: the multi-opening of n leaves, read-only — the tree is unchanged in every stored byte, its
 * root, its stats and its mode, in both modes. d_keys = n strictly increasing leaf indices below 2^H (what pw_memory_tree_update
 * takes). d_payloads (n x 8 words, row-major, Montgomery): row j = the payload stored for key j, 8 zeros where the key is not stored
 * (so an opening proves non-membership too). d_siblings (cap_siblings x 8 words, Montgomery): with T_0 = the keys and T_(l+1) =
 * unique(T_l >> 1), for l = 0 .. H - 1 in ascending level and inside a level in ascending index, for every node t of T_l whose
 * sibling t ^ 1 is NOT in T_l the digest of node (l, t ^ 1), Z_l where that node is not stored — the standard multiproof; *n_siblings
 * = their number (one key: H; the keys {0, 1}: H - 1; every leaf of a tree: 0; never above n H). Three launches whatever H is: one
 * lane per (level, key) flags the nodes whose sibling is carried, one scan ranks them, the flagged lanes look the sibling up in its
 * level and write it at its rank; nothing is hashed and no byte depends on an order of arrival. *status: 0 = written; 4 = the keys
 * are not strictly increasing or one is >= 2^H, *info = the index of the first offender (the rule of the update); 1 = cap_siblings <
 * *n_siblings (which is set). With a non-zero *status neither output buffer is touched and 0 is returned. -1 before any GPU call: a
 * NULL pointer, n == 0 (or above 2^40), changed round constants, a tree whose buffers live on another device. An empty tree may get
 * its Z_0 .. Z_H buffer allocated by this call (every sibling is a Z_l, every payload zero). The stream contract is the update's:
 * the calling thread's launch stream, a synchronisation before the return, the scratch (9 n H bytes and the scan's) freed on every
 * path. WHAT IT PROVES: that the tree with this root holds these payloads at these keys — a statement about a root. That the root is
 * the memory an execution ended with is what pw_verify_segment_chain says about the last segment's root_after.
 * pw_memory_opening_verify (host, no GPU call; the installed table): recomputes the root bottom-up from keys, payloads and siblings
 * — all canonical words, the siblings consumed in the order above — leaf = compress(payload | 0^8), node = compress(left | right).
 * 0 = the root is `root`; 20 = it is not; 19 = malformed: height outside 1 .. 40, n == 0 or a NULL pointer, the keys not strictly
 * increasing or >= 2^height (*where = the first such key's index), a word >= p (*where = its index in its array, looked for in
 * root, payloads, siblings in this order), m not the number the keys imply (*where = that number: m is derived, never trusted).
 * where may be NULL. (10 .. 18 are the proof verifiers' codes.) */
typedef struct PwMemoryTree PwMemoryTree;
typedef struct PwMemoryTreeStats {
    uint64_t leaves, stored_nodes, device_bytes;
    uint64_t last_permutations, last_launches, last_scratch_bytes;
} PwMemoryTreeStats;
PwMemoryTree* pw_memory_tree_create(uint32_t height);
void pw_memory_tree_destroy(PwMemoryTree* tree);
int pw_memory_tree_root(const PwMemoryTree* tree, uint32_t* out);
int pw_memory_tree_stats(const PwMemoryTree* tree, PwMemoryTreeStats* out);
int pw_memory_tree_update(PwMemoryTree* tree, const uint64_t* d_keys, const uint32_t* d_init, const uint32_t* d_fin, size_t n,
                          uint32_t* d_records, uint64_t* d_node_ids, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_rows,
                          uint32_t* status, uint64_t* info);
#define PW_MEMORY_TREE_REBUILD 0u
#define PW_MEMORY_TREE_INCREMENTAL 1u
int pw_memory_tree_set_mode(PwMemoryTree* tree, uint32_t mode);
int pw_memory_tree_get_mode(const PwMemoryTree* tree, uint32_t* mode);
int pw_memory_tree_boundary_leaves(const uint32_t* d_boundary_trace, uint32_t log_height, uint64_t n_locations, uint64_t* d_keys,
                                   uint32_t* d_init, uint32_t* d_fin);
int pw_memory_tree_open(const PwMemoryTree* tree, const uint64_t* d_keys, size_t n, uint32_t* d_payloads, uint32_t* d_siblings,
                        uint64_t cap_siblings, uint64_t* n_siblings, uint32_t* status, uint64_t* info);
int pw_memory_opening_verify(uint32_t height, const uint32_t* root, const uint64_t* keys, const uint32_t* payloads, size_t n,
                             const uint32_t* siblings, size_t m, size_t* where);

/* ---- the memory Merkle AIR's trace (the AIR: powdr_amd/memory_tree.py merkle_air) ------------------------------------
 * d_records (25 columns, column-major with pitch 2^records_log_height, Montgomery) and d_node_ids are what ONE pw_memory_tree_update
 * of a tree of `height` H wrote: n_rows rows (even), the first half phase 0 and the second half phase 1, both halves in the same node
 * order, the ids strictly increasing inside a half. d_trace_out (55 x 2^cap_log_height words) receives ONE row per touched node:
 *   [valid, is_root, is_leaf, left_touched, right_touched, level, index, left0[8], right0[8], out0[8], left1[8], right1[8], out1[8]]
 * column-major with pitch 2^*log_height, Montgomery; *n_nodes = n_rows / 2, *log_height = the smallest height >= 1 that holds them.
 * Row r is node *n_nodes - 1 - r of the records order, so the root is row 0 and the leaves come last; left0 / right0 / out0 are the
 * node's phase-0 record, left1 / right1 / out1 its phase-1 record; level and index come from the id; is_root on the node (H, 0),
 * is_leaf on level 0; left_touched / right_touched say whether the child (level - 1, 2 index) / (level - 1, 2 index + 1) has a row of
 * its own. Rows past *n_nodes are all zero. No byte depends on an order of arrival.
 * *status: 0 = written; 1 = cap_log_height too small (*log_height says what is needed, nothing is written); 2 = n_rows == 0 — a
 * segment that touches no memory has no root row: the AIR has no trace for it, and proving such a segment's memory continuity is out
 * of scope here (nothing is written); 3 = the ids are not a records set: the phase-1 id of some node is not its phase-0 id with bit
 * 63 set, a level is above H or an index does not fit its level, or the last id is not (H, 0) — checked on the device and read back
 * with the call's one synchronisation; the buffer then holds nothing the caller can rely on.
 * -1 before any GPU call: a NULL pointer, an odd n_rows, H outside 1 .. 30 (an index below 2^30 is a field element; the tree itself
 * allows up to 40), a log height outside 1 .. 38 (one lane per row: what a launch holds), more rows than 2^records_log_height. The call runs on the calling thread's launch
 * stream, synchronises once before it returns and frees its scratch on every path (the contract of pw_memory_boundary_trace). */
int pw_memory_merkle_trace(const uint32_t* d_records, uint32_t records_log_height, const uint64_t* d_node_ids, uint64_t n_rows,
                           uint32_t height, uint32_t* d_trace_out, uint32_t cap_log_height, uint32_t* log_height, uint64_t* n_nodes,
                           uint32_t* status);

/* Device memory ONE proof call may plan for (bytes; 0 = no limit beyond what the device has free — the default, or
 * POWDR_DEVICE_BUDGET_BYTES read once). It is applied per call, to what that call's provers and (segments) the calling thread's
 * segment context hold: a proof whose resident buffers would exceed it runs streamed (one-AIR proofs: pw_prover_prove; segments:
 * the largest AIRs first), exactly as when the device itself is short. Calls that run at the same time each get the whole budget:
 * an embedder that shares a GPU between engines sets this instead of relying on hipMemGetInfo at the moment of the call, and one
 * that runs N proofs at once on a device sets its share divided by N. */
void pw_set_device_budget(size_t bytes);
size_t pw_get_device_budget(void);

/* INDEPENDENT proofs, one per AIR (v0 / v0+LogUp), proven concurrently: `n_workers` host threads (0 = 4), each with its
 * own HIP stream on the caller's device, take the AIRs largest first; n_workers = 1 runs inline on the calling thread's
 * stream. This is the flow AIR-level sharding over several GPUs uses (every rank proves its AIRs; powdr_amd/sharding.py).
 * shared_bus_seed != 0: every prover must come from pw_prover_create_logup; phase 1 commits all traces, the bus seed is
 * pw_commitment_digest over the trace roots in AIR order, phase 2 proves every AIR with it (each prover reuses its
 * phase-1 LDE and tree). proofs[i] / n_words[i] are owned by airs[i].prover and valid until its next proof; bus_seed8
 * (may be NULL) receives the seed. Stream contract: the worker streams wait for everything the caller enqueued on its
 * launch stream before the call. Returns 0 or the first error. */
int pw_prove_airs(const PwSegmentAir* airs, size_t n_airs, int shared_bus_seed, unsigned n_workers,
                  const uint32_t** proofs, size_t* n_words, uint32_t* bus_seed8);

typedef struct PwAirDescription {
    uint32_t width, log_height;
    uint32_t logup;                                          /* 0: constraints-only ("PWS1") proof, interaction fields unused */
    const uint32_t* cons_bytecode; size_t bytecode_len;
    const uint32_t* cons_spans; size_t n_constraints;
    const uint32_t* interactions; size_t n_interactions;
    const uint32_t* inter_spans; size_t n_inter_spans;
    const uint32_t* inter_bytecode; size_t inter_bytecode_len;
} PwAirDescription;

/* Host verification (no GPU) of a pw_prove_segment proof: the counterpart of `verify_app_proof` for a whole segment.
 * airs[i].logup is ignored (the segment's `logup` flag applies to all). Returns 0 = valid; ((air index + 1) << 8) | 2 =
 * constraint identity of that AIR; 1 header / shape mismatch, 3 proof of work, 4 query index, 5 main opening,
 * 6 quotient opening, 7 FRI layer, 8 final value, 9 trailing words, 10 truncated, 11 permutation opening, 13 a word >= p,
 * 14 check_balance is set and the AIRs' cumulative bus sums do not add up to zero, 15 malformed description.
 * total_sum4 (may be NULL) receives the sum of the cumulative sums. */
int pw_verify_segment(const PwStarkConfig* cfg, const PwAirDescription* airs, size_t n_airs, int logup,
                      const uint32_t* proof_words, size_t n_words, int check_balance, uint32_t* total_sum4);

/* The verifying key's part of an AIR with preprocessed columns: their number and pw_prover_preprocessed_root (canonical);
 * width = 0: the AIR has none. */
typedef struct PwAirPreprocessed {
    uint32_t width;
    uint32_t root8[8];
} PwAirPreprocessed;

/* pw_verify_segment for segments whose AIRs may have preprocessed columns (pre: one entry per AIR; NULL or every width 0 = exactly
 * pw_verify_segment). Column operands of the descriptions below width + pre[i].width are valid. Additional code 16 = a preprocessed
 * row does not open against its root; a PWS3 proof checked against a description that claims preprocessed columns, or a PWS4 proof
 * against one that claims none, returns 1. */
int pw_verify_segment_preprocessed(const PwStarkConfig* cfg, const PwAirDescription* airs, const PwAirPreprocessed* pre, size_t n_airs,
                                   int logup, const uint32_t* proof_words, size_t n_words, int check_balance, uint32_t* total_sum4);

/* pw_verify_segment_preprocessed for segments whose AIRs may be row-aware (pw_prover_create_transition; pre may be NULL). Constraint
 * operands below 2 (width + pre[i].width) + 3 and interaction operands below width + pre[i].width are valid, anything else returns 15.
 * The row flags of every AIR are derived from its constraint programs; a PWS5 proof against descriptions with no row-aware AIR, or
 * another proof against descriptions with one, returns 1. Without a row-aware AIR: exactly pw_verify_segment_preprocessed. */
int pw_verify_segment_transition(const PwStarkConfig* cfg, const PwAirDescription* airs, const PwAirPreprocessed* pre, size_t n_airs,
                                 int logup, const uint32_t* proof_words, size_t n_words, int check_balance, uint32_t* total_sum4);

/* The public values of one AIR as the verifier is told them (one entry per AIR of a segment): n = how many the AIR has
 * (0: none; it comes from the description, never from the proof), expected = what they must be (canonical), NULL = accept what the proof
 * carries (pw_segment_proof_public_values reads them out). */
typedef struct PwAirPublic {
    uint32_t n;
    const uint32_t* expected;
} PwAirPublic;

/* pw_verify_segment_transition for segments whose AIRs may have public values (pub == NULL or every n == 0: exactly that function).
 * Constraint operands below 2 (width + pre[i].width) + 3 + pub[i].n are valid; an AIR with public values is held to what its prover entry
 * checks (a constraint of degree > 3, an interaction operand at or above width + pre[i].width, n > 256: 15). The values enter the
 * transcript and the constraint identity at zeta. Additional code 17 = the proof's public values of some AIR differ from `expected`;
 * a PWS6 proof against descriptions without public values, or another proof against descriptions with some, returns 1. */
int pw_verify_segment_public(const PwStarkConfig* cfg, const PwAirDescription* airs, const PwAirPreprocessed* pre, const PwAirPublic* pub,
                             size_t n_airs, int logup, const uint32_t* proof_words, size_t n_words, int check_balance, uint32_t* total_sum4);
/* AIR `air`'s public values as a proof carries them: up to `cap` canonical words to `out` (may be NULL), returns their number
 * (pub[air].n). (size_t)-1: the proof's header does not match the descriptions (nothing else of the proof is looked at: verify it). */
size_t pw_segment_proof_public_values(const PwAirDescription* airs, const PwAirPublic* pub, size_t n_airs, const uint32_t* proof_words,
                                      size_t n_words, size_t air, uint32_t* out, size_t cap);

/* N segment proofs are CONSECUTIVE pieces of one execution: every segment verifies (pw_verify_segment_public) and every link holds from
 * each segment to the next — link {air_from, index_from, air_to, index_to}: public value index_from of AIR air_from in segment s equals
 * public value index_to of AIR air_to in segment s + 1, for every s < n_segments - 1 (the connector's final state = the next connector's
 * initial state). Returns 0; the segment verifier's code of the first failing segment with *where = its index; 18 = a link does not hold
 * (or names a value the descriptions do not have), *where = s * n_links + link. Host only. `where` may be NULL.
 * NOT checked: that all segments ran the same program — compare the `pre` root of the program AIR across the segments; that is the caller's. */
typedef struct PwChainSegment {
    const PwAirDescription* airs;
    const PwAirPreprocessed* pre;   /* may be NULL */
    const PwAirPublic* pub;         /* may be NULL */
    size_t n_airs;
    int logup;
    const uint32_t* proof;
    size_t n_words;
    int check_balance;
} PwChainSegment;
typedef struct PwChainLink {
    uint32_t air_from, index_from, air_to, index_to;
} PwChainLink;
int pw_verify_segment_chain(const PwStarkConfig* cfg, const PwChainSegment* segments, size_t n_segments, const PwChainLink* links,
                            size_t n_links, size_t* where);

/* Host verification of pw_prove_airs' proofs. With shared_bus_seed the seed is recomputed from the trace roots inside the
 * proofs and every proof must have used it. Returns 0; ((air index + 1) << 8) | code of the first failing proof
 * (codes as pw_verify / pw_verify_logup); or 14 when check_balance is set and the cumulative bus sums of all AIRs
 * do not add up to zero. total_sum4 (may be NULL) receives that sum. */
int pw_verify_airs(const PwStarkConfig* cfg, const PwAirDescription* airs, size_t n_airs,
                   const uint32_t* const* proofs, const size_t* n_words, int shared_bus_seed, int check_balance,
                   uint32_t* total_sum4);

/* ---- independent segments over the GPUs of one node ------------------------------------------------------------------
 * The reference proves an execution's segments one after the other on one device (openvm/src/trace_generation.rs:111-141);
 * they are independent once metered execution has fixed their boundaries. pw_prove_segments_multi runs that loop on
 * `n_workers` host threads at once: worker w makes devices[w] current, gets a launch stream of its own and proves the
 * segments placed on it — by `segment_cells` (rows x columns), largest first, each to the least loaded worker
 * (pw_assign_units) — by calling `prove(user, segment, worker, device, commitment8)`: the caller's per-worker replica of the
 * segment pipeline (trace generation into that worker's buffers, pw_prove_segment on that worker's provers; a prover belongs
 * to the device it was created on) which returns the segment's 8-word main commitment (canonical; proof words 5 + 4 n_airs
 * .. + 8 of a pw_prove_segment proof) and keeps or ships the proof itself. No data-path collective. Afterwards the FINAL
 * COMMITMENT MERGE: the commitments are all-gathered over RCCL (one rank per distinct device; workers may share a device) and
 * `commitments` (n_segments x 8 words, host) receives the segment-ordered list every device now holds. RCCL is loaded with
 * dlopen; without it (or POWDR_MULTI_NO_RCCL=1) the merge happens on the host — pw_multi_last_merge(): 1 = RCCL, 2 = host.
 * worker_of_segment (may be NULL) receives who proved each segment in the end. The placement by cells is the PLAN (pw_assign_units):
 * a worker whose queue runs dry steals the smallest unstarted segment of the worker with the most cells still queued — proving time is
 * not proportional to cells (short tails, streamed AIRs) and devices differ by a few percent; POWDR_MULTI_STEAL=0 keeps the plan.
 * Returns 0, the first error of a worker, or a hipError_t. */
typedef int (*PwSegmentProveFn)(void* user, size_t segment, size_t worker, int device, uint32_t* commitment8);
int pw_prove_segments_multi(const int* devices, size_t n_workers, const uint64_t* segment_cells, size_t n_segments,
                            PwSegmentProveFn prove, void* user, uint32_t* commitments, uint32_t* worker_of_segment);
int pw_multi_last_merge(void);
/* Largest-first greedy balance of `n_units` proof units over `n_workers` (ties: lower unit index, lower worker index first);
 * worker_of_unit[u] = the worker unit u is placed on. Returns n_units (0: malformed arguments). */
size_t pw_assign_units(const uint64_t* cells, size_t n_units, size_t n_workers, uint32_t* worker_of_unit);

/* Digest over an ordered list of 8-word commitments (binary Poseidon2 tree; canonical words). */
void pw_commitment_digest(const uint32_t* roots8, size_t n, uint32_t* digest8);

/* Set-up for proofs of 2^log_height-row traces, so that the first pw_prover_prove pays for neither: (1) the run-time specialised
 * kernels are compiled now if the height policy would compile them at the first proof (seconds of host time for a keccak-sized AIR;
 * their partial-sum buffer is part of the reservation), (2) every device buffer such a proof needs is allocated (tens of gigabytes
 * for wide traces) — in the mode the memory free NOW allows (resident, or streamed: see below). Buffers only grow; calling it is
 * optional. Returns hipErrorOutOfMemory when not even the streamed buffers fit. */
int pw_prover_reserve(PwProver* p, uint32_t log_height);

/* STREAMED proofs. A resident proof keeps the low-degree extension of every committed column in HBM (8 bytes per committed cell
 * next to the caller's trace); BASELINE configs[2] — the reference's default segment height 2^22
 * (/root/reference/openvm-riscv/src/lib.rs:366-371) with the bus interactions PowdrAir::eval always pushes
 * (/root/reference/openvm/src/powdr_extension/chip.rs:117-129) — would need 280 GB for 3 731 + 4 632 columns. When that does not
 * fit, pw_prover_prove / pw_prover_trace_root / pw_prover_reserve switch to the streamed mode by themselves: the prover keeps the
 * columns' COEFFICIENT arrays (4 bytes per committed cell) and walks the extended domain as 2^b sub-cosets (rows r + 2^b i),
 * rebuilding the LDE rows of all columns for one sub-coset at a time — for the leaf hashes of the commitments, for the quotient and
 * for the query answers. Same proof words as the resident mode. POWDR_STREAM_LOG_BLOCKS=0 forces resident, =b (>= 1) streamed.
 * pw_prover_stream_log_blocks: the mode a proof of a 2^log_height-row trace would run in with the memory free NOW — 0 resident,
 * b >= 1 streamed over 2^b sub-cosets, -1 not even that fits. */
int pw_prover_stream_log_blocks(const PwProver* p, uint32_t log_height);

/* Highest degree (in the trace columns) among the constraint programs the prover was created with; 99 if one of them
 * is malformed or not polynomial. The blow-up-2 quotient carries degree <= 3 — the reference's bound
 * 2 * DEFAULT_APP_LOG_BLOWUP + 1 (openvm/src/lib.rs:97-101); a prover with a higher value produces proofs that do not
 * verify, so a key generator checks this once. */
int pw_prover_max_constraint_degree(const PwProver* p);

/* Run-time specialised expression kernels. The constraint and interaction programs of a prover are wave-uniform bytecode that
 * the ahead-of-time kernels interpret; for an AIR that is proven segment after segment the library can instead emit them as
 * straight-line HIP, compile that with hiprtc for gfx950 (translation units concurrently on host threads; hiprtc is loaded
 * with dlopen, the library works without it) and run the code objects for the quotient and the LogUp permutation columns.
 * Same proof words either way. By default a prover is specialised at its first proof of a trace of at least 2^18 rows
 * (POWDR_JIT_MIN_LOG_HEIGHT), which costs seconds of host time once; POWDR_JIT=0 never, POWDR_JIT=1 at every first proof.
 * pw_prover_specialise does it now (set-up time, like pw_prover_reserve): 0 = the prover has specialised kernels, 1 = it
 * keeps the interpreter (no hiprtc, POWDR_JIT=0, programs that did not compile to xbc, a compiler error).
 * pw_prover_specialised returns the state (1 specialised, 0 not tried yet, -1 interpreter only) and the number of compiled
 * kernels, their code-object bytes and the number of code chunks (each NULL = skip). */
int pw_prover_specialise(PwProver* p);
/* The same for n provers in ONE concurrent compile batch, whatever their traces' heights (an AIR set that is proven segment after
 * segment is compiled once, at set-up: the reference fixes an APC's AIR at key generation). Returns how many of them run specialised
 * kernels afterwards. Short traces gain most: an interpreted expression kernel walks the AIR's whole program in every lane — ~1.2 ms
 * per launch for a 2 000-column AIR however few rows it has (profiles/r06_tail_segment_c5.txt); measured on the reth-shaped segments
 * (61 AIRs): 5.17 -> 5.41 G cells/s for 145 s of cold compilation. */
size_t pw_provers_specialise(PwProver* const* provers, size_t n);
int pw_prover_specialised(const PwProver* p, size_t* n_kernels, size_t* code_bytes, size_t* n_chunks);
/* Test hook: the HIP source the generator emits for translation unit `unit` of an AIR's specialised kernels (which: 0 = quotient
 * numerator, 1 = LogUp permutation columns; chunk_cost / chunks_per_unit 0 = the defaults), without compiling it: lets a CPU-only
 * test build the generated code for the HOST and execute it. Returns the source length (0: no such unit). */
size_t pw_jit_generated_source(uint32_t width, const uint32_t* cons_bytecode, size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints,
                               const uint32_t* interactions, size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                               const uint32_t* inter_bytecode, size_t inter_bytecode_len, int which, uint32_t chunk_cost, uint32_t chunks_per_unit,
                               size_t unit, char* buf, size_t cap, char* kernel_name, size_t name_cap, uint32_t* first_chunk, uint32_t* n_chunks,
                               uint32_t* total_chunks);
/* Compiled code objects are kept on disk across processes: $POWDR_JIT_CACHE_DIR, else $XDG_CACHE_HOME/powdr_jit, else
 * $HOME/.cache/powdr_jit (POWDR_JIT_CACHE=0: off); an entry is keyed by the unit's source, the embedded headers and the compile options
 * and confirmed by comparing the stored source. Translation units this process compiled / loaded from disk so far: */
void pw_jit_cache_stats(uint64_t* units_compiled, uint64_t* units_from_disk);
/* The same code generation + hiprtc compilation for an AIR given by its tables (as for pw_prover_create / _create_logup;
 * interactions == NULL: constraints only) WITHOUT touching a GPU — hiprtc cross-compiles — so build machines and CPU test
 * suites can check that an AIR's specialised kernels compile. Returns pw_prover_specialise's code (-2: malformed tables);
 * err (may be NULL) receives the compiler's message. */
int pw_jit_compile_check(uint32_t width, const uint32_t* cons_bytecode, size_t bytecode_len, const uint32_t* cons_spans, size_t n_constraints,
                         const uint32_t* interactions, size_t n_interactions, const uint32_t* inter_spans, size_t n_inter_spans,
                         const uint32_t* inter_bytecode, size_t inter_bytecode_len, size_t* n_kernels, size_t* code_bytes, size_t* n_chunks,
                         char* err, size_t err_cap);

/* Number of main-trace columns the prover was created for. */
uint32_t pw_prover_width(const PwProver* p);

/* Bytes of device memory the prover currently holds. */
size_t pw_prover_device_bytes(const PwProver* p);

/* ---- single stages, exposed for parity tests and per-stage measurement ---- */

/* d_coeffs (width x H) receives H-scaled coefficients in bit-reversed order; d_lde (width x 2H)
 * receives natural-order evaluations on the coset 31 * <g_{n+1}>. */
int pw_lde_batch(const uint32_t* d_trace, uint32_t width, uint32_t log_height, uint32_t* d_coeffs, uint32_t* d_lde);

/* The same LDE the way the provers run it: three passes over HBM instead of four — the contiguous stage groups of the
 * inverse and of the forward transform share one kernel, the coefficient array is never written (d_tmp: width x H words of
 * scratch for the strided stages of traces taller than 2^12 rows; its contents are unspecified afterwards). */
int pw_lde_fused(const uint32_t* d_trace, uint32_t width, uint32_t log_height, uint32_t* d_tmp, uint32_t* d_lde);

/* One sub-coset of the LDE from coefficient arrays (the stage the streamed mode is built on): d_coeffs as pw_lde_batch leaves them
 * (width x H, bit-reversed, H-scaled); d_out (width x 2H / 2^log_blocks) receives the rows r + 2^log_blocks * i of the LDE, i.e. the
 * evaluations on (31 g_(n+1)^r) <g_(n+1)^(2^log_blocks)>; d_scale: H words of scratch. 1 <= log_blocks <= min(log_height, 5). */
/* d_coeffs must be 16-byte aligned (hipErrorInvalidValue otherwise). */
int pw_lde_subcoset(const uint32_t* d_coeffs, uint32_t width, uint32_t log_height, uint32_t log_blocks, uint32_t r, uint32_t* d_scale,
                    uint32_t* d_out);

/* Poseidon2 Merkle tree of a column-major matrix; d_digests gets (2*height - 1) * 8 words,
 * leaves first, root last. */
int pw_merkle_commit(const uint32_t* d_matrix, size_t height, uint32_t width, uint32_t* d_digests);

/* The commitment kernels form by form. Every call validates its arguments first and launches nothing when it refuses: -1 for a
 * malformed argument (a NULL pointer where one is needed, a zero height / width / n_cols, and what each call lists below),
 * hipErrorInvalidValue for a digest or state pointer that is not 16-byte aligned (the kernels store 16 bytes at a time). Words on the
 * device are Montgomery words, as everywhere.
 *
 * Row digests of a column-major matrix (any height >= 1, column c at d_matrix + c * col_stride, col_stride >= height): the digest of
 * row j goes to the 8 words at slot j * digest_stride + digest_offset of d_digests (digest_offset < digest_stride), so a matrix that
 * holds the rows r + 2^b i of a committed one fills its share of the leaves with (2^b, r). Other slots are not written. */
int pw_merkle_leaf_hash(const uint32_t* d_matrix, size_t height, uint32_t width, size_t col_stride, uint32_t* d_digests,
                        size_t digest_stride, size_t digest_offset);

/* One RUN of the row digests of a level whose hashed row is the concatenation of several matrices' rows. The run's n_cols columns are
 * those of a matrix (d_matrix, col_stride >= height) or of a device array of n_cols device column pointers (d_cols): exactly one of
 * the two. Row j < height of the run is row j * row_stride + row_offset of the level (row_offset < row_stride). pos0 < 8 = the number
 * of columns the level's earlier runs absorbed, mod 8. first: the sponge states start at zero (pos0 must be 0); otherwise they are
 * read from d_state (16 words per row of the level). last: the digests are written to d_digests (8 words per row of the level);
 * otherwise the states go back to d_state, as words that only a later run of the same level can read. Rows the run does not name are
 * not touched. Same digests as one sponge over the whole row. */
int pw_merkle_leaf_absorb(const uint32_t* d_matrix, size_t col_stride, const uint32_t* const* d_cols, uint32_t n_cols, uint32_t pos0,
                          size_t height, size_t row_stride, size_t row_offset, uint32_t* d_state, uint32_t* d_digests, int first, int last);

/* The mixed-height tree of a segment commitment over the levels of 2^L, ..., 1 rows. n_cols_by_log[k] and external_by_log[k], k = 0..L
 * (host arrays): the number of columns of height 2^k, and whether the level's row digests are already in place (level L: the first
 * 2^L * 8 words of d_digests; level k < L: d_inject + 2^k * 8) instead of being hashed here. d_cols: ONE device array of device column
 * pointers, level L's n_cols_by_log[L] first, then level L - 1's, ..., level 0's last (an external level's entries are skipped, not
 * read; NULL if every populated level is external). Level L must be populated or external; L <= 27. d_digests: (2^(L+1) - 1) * 8 words,
 * the levels of 2^L, 2^(L-1), ..., 1 nodes back to back: node j of the level of n nodes = compress(child j, child j + n), then, where
 * the level is populated or external, compress(node, digest of row j). d_inject: 2^L * 8 words of scratch (NULL if no level below L is
 * populated or external). */
int pw_merkle_commit_mixed(const uint32_t* const* d_cols, const uint32_t* n_cols_by_log, const uint32_t* external_by_log, uint32_t L,
                           uint32_t* d_digests, uint32_t* d_inject);

/* The tree of a FRI round: d_values = 2 * half extension elements (4 words each), leaf i = the first 8 words of
 * Poseidon2(v[i] || v[i + half] || 0^8), then the binary tree; half a power of two; d_digests gets (2 * half - 1) * 8 words. */
int pw_merkle_commit_ext_pairs(const uint32_t* d_values, size_t half, uint32_t* d_digests);

/* ---- single stages: the opening, DEEP, FRI, scan and layout kernels ----
 *
 * One entry point per kernel (family) between the commitments and the proof words, for kernel-level tests and per-stage measurement;
 * an engine never calls them. Conventions of every call below:
 *   - device matrices and vectors hold Montgomery words, matrices column-major; an extension element is 4 consecutive words;
 *   - extension scalars (zeta, gzeta, beta, sum, sum1, sum2, gK, base, a) are HOST pointers to 4 canonical words;
 *   - tables of opening weights and of gamma powers (d_w, d_w2, d_gpow, d_gq) are device arrays in the form the kernels consume:
 *     per element 4 int32, the centred representatives (|.| <= (p - 1) / 2) of the element's Montgomery words. pw_stage_opening_weights
 *     and pw_stage_ext_powers(centred = 1) write that form; a caller may pass any table of it;
 *   - a call launches on the calling thread's stream and does not wait, except pw_stage_ext_dot and pw_stage_logup_scan, which own
 *     scratch and release it before they return (they wait for the stream first);
 *   - -1, before anything is launched: a NULL pointer where one is needed, a scalar word >= p, a log size out of range, a zero size,
 *     and what a call lists; otherwise 0 or a HIP error code (hipErrorInvalidValue = 1 where a call says so).
 * x_j = 31 * w^j with w the generator of the order-2^log_n subgroup is row j of the extended domain. */

/* d_w[i] (2^log_h elements), log_h <= 26. on_coefficients = 0: the barycentric weights ((zeta^H - 1) / H) g^i / (zeta - g^i) of the
 * trace domain, f(zeta) = sum_i f(g^i) w[i]; 1: zeta^bitrev(q) / H, for the coefficient arrays pw_lde_batch leaves. */
int pw_stage_opening_weights(const uint32_t* zeta, uint32_t log_h, int on_coefficients, uint32_t* d_w);

/* d_out[c] = sum_{q < len} d_w[q] * column c [q], column c at d_cols + c * stride (stride >= len), c < n_cols; with d_w2 (may be
 * NULL) also d_out2[c] for the second weight vector, in the same pass. d_w / d_w2 not 16-byte aligned: hipErrorInvalidValue. */
int pw_stage_ext_dot(const uint32_t* d_cols, size_t stride, uint32_t n_cols, size_t len, const uint32_t* d_w, const uint32_t* d_w2,
                     uint32_t* d_out, uint32_t* d_out2);

/* d_out[k] = base^k, or base^(n - 1 - k) when reversed, k < n; centred: in the table form above, else as Montgomery words.
 * n > 2^24: hipErrorInvalidValue. */
int pw_stage_ext_powers(const uint32_t* base, uint32_t n, int reversed, int centred, uint32_t* d_out);

/* d_v[j] = (sum_{k < wa} g[k] a_k[j] + sum_{k < wb} g[wa + k] b_k[j] - sum) / (x_j - zeta), j < 2^log_n, for two matrices of wa and wb
 * columns of 2^log_n rows (any widths, not both zero); 1 <= log_n <= 27; g = d_gpow, wa + wb elements. */
int pw_stage_deep(const uint32_t* d_a, uint32_t wa, const uint32_t* d_b, uint32_t wb, uint32_t log_n, const uint32_t* d_gpow,
                  const uint32_t* sum, const uint32_t* zeta, uint32_t* d_v);

/* The two-term form over the main (W columns), permutation (Wp) and quotient (8) matrices, K1 = W + Wp + 8, g = d_gpow (K1 + Wp elements):
 *   A1 = sum_{k < W} g[k] f_k + sum_{k < Wp} g[W + k] p_k + sum_{k < 8} g[W + Wp + k] q_k,   A2 = sum_{k < Wp} g[K1 + k] p_k,
 *   d_v[j] = (A1[j] - sum1) / (x_j - zeta) + (A2[j] - sum2) / (x_j - gzeta).
 * With gK (may be NULL) the two-point form: A2 += gK * sum_{k < W} g[k] f_k. Wp = 0 (d_plde NULL) is allowed. */
int pw_stage_deep_logup(const uint32_t* d_lde, uint32_t W, const uint32_t* d_plde, uint32_t Wp, const uint32_t* d_qlde, uint32_t log_n,
                        const uint32_t* d_gpow, const uint32_t* gK, const uint32_t* sum1, const uint32_t* sum2, const uint32_t* zeta,
                        const uint32_t* gzeta, uint32_t* d_v);

/* d_out = 4 columns of len words, the coordinates of sum_{k < wa} g[k] a_k + sum_{k < wb} g[wa + k] b_k; with second != 0 four more,
 * those of sum_{k < wb} g[second + k] b_k. An odd len, or d_a / d_b / d_out not 8-byte aligned: hipErrorInvalidValue. */
int pw_stage_ext_lincomb(const uint32_t* d_a, uint32_t wa, const uint32_t* d_b, uint32_t wb, size_t len, const uint32_t* d_gpow, uint32_t second,
                         uint32_t* d_out);

/* d_v[j] = (G1[j] + sum_{k < 8} gq[k] q_k[j] - sum1) / (x_j - zeta) [+ (G2[j] - sum2) / (x_j - gzeta) when two]; d_glde = the four
 * coordinate columns of G1, then those of G2 (8 columns of 2^log_n; the last four are not read unless two). */
int pw_stage_deep_from_combo(const uint32_t* d_glde, const uint32_t* d_qlde, uint32_t log_n, const uint32_t* d_gq, const uint32_t* sum1,
                             const uint32_t* sum2, const uint32_t* zeta, const uint32_t* gzeta, int two, uint32_t* d_v);

/* One FRI round: d_out[i] = (a + b) / 2 + beta (a - b) / (2 shift w^i), a = d_v[i], b = d_v[i + half], i < half = 2^(log_size - 1), w of
 * order 2^log_size; shift: a canonical non-zero base-field word; 1 <= log_size <= 27. */
int pw_stage_fri_fold(const uint32_t* d_v, uint32_t log_size, uint32_t shift, const uint32_t* beta, uint32_t* d_out);

/* Inclusive prefix sums of H extension elements into four columns: d_phi_cols[k * H + r] = coordinate k of sum_{i <= r} d_rowsum[i]. */
int pw_stage_logup_scan(const uint32_t* d_rowsum, size_t H, uint32_t* d_phi_cols);

/* The quotient's two chunks from the unscaled DIF-iNTT of its four coordinate columns over N = 2H points (d_cbr: 4 x N):
 * d_out[(4 ch + k) H + q] = d_cbr[k N + 2 q + ch] * 31^-(bitrev(q) + ch H) / 2 (8 x H). d_cbr not 8-byte aligned: hipErrorInvalidValue. */
int pw_stage_quotient_split(const uint32_t* d_cbr, uint32_t log_h, uint32_t* d_out);

/* The row layout behind the w1 columns of the n = 2^log_n-row matrix d_m (column stride n), in place: column w1 + i = column
 * d_next_cols[i] (a device array, entries < w1) moved up by `step` rows, cyclically, i < n_next; then, when selectors, is_first_row,
 * is_last_row and is_transition on the rows' points: x_j of the extended domain (trace_domain = 0; the trace has n / 2 rows) or the
 * trace domain's own g^j (1). */
int pw_stage_row_layout(uint32_t* d_m, uint32_t log_n, uint32_t w1, const uint32_t* d_next_cols, uint32_t n_next, uint32_t step, int selectors,
                        int trace_domain);

/* d_out[k N + r + (i << b)] = sum_{c < n_chunks} d_part[(4 c + k) m + i] mod p, k < 4, i < m (plain sums of words: canonical in,
 * canonical out). r < 2^b and r + 2^b (m - 1) < N, else -1. */
int pw_stage_part_scatter(const uint32_t* d_part, uint32_t n_chunks, size_t m, uint32_t b, uint32_t r, size_t N, uint32_t* d_out);

/* d_y[i] += a * d_x[i] over n extension elements; a NULL: a = 1. */
int pw_stage_ext_axpy(uint32_t* d_y, const uint32_t* a, const uint32_t* d_x, size_t n);

/* ---- single stages: the LogUp permutation trace and the quotient ----
 *
 * The conventions above hold. These take a prover, because the programs live there, and run the path THAT prover would run in a proof:
 * its run-time specialised kernels if it has them (pw_prover_specialise), else the interpreter kernels — small forms, or post-fix
 * where the prover was created with POWDR_LOGUP_INTERPRET=1 / POWDR_QUOTIENT_XBC=0. Every path computes the same words. The challenge
 * TABLES are the caller's device arrays of Montgomery extension elements, nominally powers of a challenge, but any table is taken:
 *   d_blpow: max_args + 2 elements, beta^0 .. — argument j of an interaction meets d_blpow[j + 1];
 *   d_apow:  one element per folded constraint: the n_constraints programs, then (LogUp) the G groups, then is_first, is_transition,
 *            is_last — alpha_c^(M - 1) .. alpha_c^0 in a proof.
 * `alpha` here is the BUS challenge: d_i = alpha + bus_i + sum_j d_blpow[j + 1] a_ij. G = the prover's LogUp groups
 * (pw_logup_group_starts). -1 also for a prover with preprocessed columns, a row layout or public values (whole proofs cover those),
 * for a LogUp call on a prover without interactions and the reverse. The specialised kernels keep their partial sums in the prover's
 * own scratch, so one prover serves one such call at a time. */

/* The permutation trace of 2^log_h rows (log_h <= 26) of d_values (the prover's columns, column-major): d_perm[(4 g + k) H + r] =
 * coordinate k of q_g(r) = sum_{i in g} m_i(r) / d_i(r) — one shared inversion per group, the inverse of 0 being 0 —, then the 4
 * columns of phi(r) = sum_{r' <= r} sum_g q_g(r'); d_rowsum[r] = sum_g q_g(r), H elements. A specialised prover also writes the row
 * sums as 4 more columns behind phi: d_perm holds 4 G + 8 columns then, else 4 G + 4. Waits for the stream (it owns scratch). */
int pw_stage_logup_perm(PwProver* p, const uint32_t* d_values, uint32_t log_h, const uint32_t* alpha, const uint32_t* d_blpow, uint32_t* d_perm,
                        uint32_t* d_rowsum);

/* The quotient over the N = 2^log_n rows (1 <= log_n <= 27) of the extended domain of a trace of H = N / 2 rows, 4 columns into d_q:
 *   acc_j = sum_c apow[c] C_c(row j) + sum_g apow[nc + g] (q_g den_g - num_g)(row j) + apow[nc + G] is_first (phi - sum_g q_g)
 *           + apow[nc + G + 1] is_transition (phi' - phi - sum_g q_g') + apow[nc + G + 2] is_last (phi - S),     d_q[k N + j] = acc_j / Z_H(x_j)
 * with den_g = prod_{i in g} d_i, num_g = sum_{i in g} m_i prod_{l != i} d_l, ' = row (j + 2) mod N, Z_H(x) = x^H - 1, g the trace
 * domain's generator and is_first = Z_H / (x - 1), is_last = Z_H / (x - 1 / g), is_transition = x - 1 / g. d_lde: the prover's columns
 * extended; d_plde: the 4 G group columns and the 4 phi columns extended. A specialised LogUp prover reads sum_g q_g from 4 more
 * columns of d_plde behind phi (the extended row sums): they must hold the sum of the group columns for the paths to agree.
 * Without interactions d_plde, alpha, d_blpow and S are NULL and only the first sum is taken. n_chunks_out (may be NULL): how many
 * partial sums were combined. The interpreter's constraints-only form owns scratch and waits for the stream. */
int pw_stage_quotient(PwProver* p, const uint32_t* d_lde, const uint32_t* d_plde, uint32_t log_n, const uint32_t* d_apow, const uint32_t* alpha,
                      const uint32_t* d_blpow, const uint32_t* S, uint32_t* d_q, uint32_t* n_chunks_out);

/* The terms of acc that read the current row alone (the first two sums), unscaled, on `rows` rows of d_T (the prover's columns) and
 * d_Pm (the 4 G group columns), column stride `rows` (1 <= rows <= 2^27): what the streamed route computes per sub-coset. The result is
 * *n_parts_out partial sums d_part[(4 c + k) rows + j] whose sum over c is the value: 1 on the interpreter paths, the chunks of the
 * specialised kernels otherwise. unit >= 0 (a specialised prover only, unit < pw_prover_quotient_units): that translation unit alone,
 * which writes the parts of its own chunks and reads only the group columns 4 g0 .. 4 g1 - 1 of its groups
 * (pw_prover_quotient_unit_groups) — d_Pm is then a PANEL of those 4 (g1 - g0) columns alone, as the streamed route extends them
 * unit by unit; the kernel is handed the address column 0 would have, d_Pm - 4 g0 rows, by the same function as there.
 * unit < 0: everything. log_n as above (the interpreter derives its unused domain constants from it). */
int pw_stage_quotient_sums(PwProver* p, const uint32_t* d_T, const uint32_t* d_Pm, size_t rows, uint32_t log_n, const uint32_t* d_apow,
                           const uint32_t* alpha, const uint32_t* d_blpow, int unit, uint32_t* d_part, uint32_t* n_parts_out);

/* Translation units of a specialised prover's quotient kernels (0: not specialised), and the LogUp groups [*g0, *g1) unit `unit`
 * reads (equal: none; -1: no such unit). */
uint32_t pw_prover_quotient_units(const PwProver* p);
int pw_prover_quotient_unit_groups(const PwProver* p, uint32_t unit, uint32_t* g0, uint32_t* g1);

/* The boundary terms and the division on top of n_chunks partial sums (plain sums of words, as pw_stage_part_scatter):
 *   d_q[k N + j] = (sum_c d_part[(4 c + k) N + j] + the three boundary terms of acc_j above, apow_tail[0 .. 2]) / Z_H(x_j)
 * with phi from d_plde_phi and sum_g q_g from d_plde_sumq (4 columns of N each). d_q may be d_part when n_chunks = 1. */
int pw_stage_logup_tail(const uint32_t* d_part, uint32_t n_chunks, const uint32_t* d_plde_phi, const uint32_t* d_plde_sumq, uint32_t log_n,
                        const uint32_t* d_apow_tail, const uint32_t* S, uint32_t* d_q);

/* d_rowsum[r] = sum_c d_part[(4 c + k) H + r] mod p as H extension elements, and the same as 4 columns d_cols4[k H + r]. */
int pw_stage_rowsum_combine(const uint32_t* d_part, uint32_t n_chunks, size_t H, uint32_t* d_rowsum, uint32_t* d_cols4);

/* ---- single stages: the query phase ----
 *
 * The conventions above hold: -1 before any launch for a NULL pointer, a zero size, a log out of range and a host word >= p; else 0 or
 * a HIP error code. Every call runs the function the provers run; none owns a kernel. Indices that live on the DEVICE (d_idx, the
 * offsets behind d_ptrs) are the caller's to keep inside the matrices, as they are the provers'. */

/* Proof of work on a transcript given by its parts, HOST arrays of canonical words: the 16 words of the sponge state and the in_len
 * (0 .. 7) observed words that are not absorbed yet. *witness_out = the SMALLEST w for which the transcript, having observed w, draws
 * `bits` zero bits — the candidates are searched 2^20 at a time. bits: 1 .. 31 — a prover hands every non-zero pow_bits to this search
 * (0 means no proof of work and no search) and a drawn word has 31 bits. Converts to Montgomery words, owns and releases its 25 words of
 * scratch, waits for the stream. hipErrorUnknown: no witness below p. */
int pw_stage_pow_grind(const uint32_t* state16, const uint32_t* pending, uint32_t in_len, uint32_t bits, uint32_t* witness_out);

/* d_out[q * width + c] = d_m[c * height + d_idx[q]], q < n_idx <= 65535 (column-major matrix, device indices below `height`); with
 * `canonical` the n_idx * width words are then taken from Montgomery to canonical form, as the proof's rows are. */
int pw_stage_gather_rows(const uint32_t* d_m, size_t height, uint32_t width, const uint32_t* d_idx, uint32_t n_idx, int canonical,
                         uint32_t* d_out);

/* d_words[i] <- the canonical representative of the Montgomery word d_words[i], i < n, in place. */
int pw_stage_canonicalize(uint32_t* d_words, size_t n);

/* The rows of MANY matrices in one launch, as a segment's query phase takes them: for every job (a HOST array of records)
 *   d_out[out_off + q * width + c] = d_m[c * height + d_idx[idx_off + q]],  q < n_idx.
 * n_jobs, n_idx <= 65535. The grid is sized by the widest job, by the helper the segment prover uses. Owns the device copy of the
 * records and waits for the stream. */
typedef struct {
    const uint32_t* d_m; /* device matrix, column-major */
    uint64_t height;
    uint32_t width;
    uint32_t idx_off;    /* this job's first index in d_idx */
    uint64_t out_off;    /* word offset of this job's rows in d_out */
} PwStageGatherJob;
int pw_stage_gather_rows_multi(const PwStageGatherJob* jobs, uint32_t n_jobs, const uint32_t* d_idx, uint32_t n_idx, uint32_t* d_out);

/* d_out[r * words_per_record + w] = d_arena[offsets[r] + w], r < n: the digests (8 words) and extension elements (4) of the query
 * answers. offsets: a HOST array of 64-bit WORD offsets into the arena; n * words_per_record < 2^32. Owns the device copy of the offsets. */
int pw_stage_gather_records(const uint32_t* d_arena, const uint64_t* offsets, uint32_t words_per_record, uint32_t n, uint32_t* d_out);

/* d_out[i] = *d_ptrs[i], i < n: d_ptrs is a DEVICE array of device pointers. */
int pw_stage_gather_words(const uint32_t* const* d_ptrs, uint32_t n, uint32_t* d_out);

/* d_cols4[k * len + q] = coordinate k of the extension element d_in[q]: a vector of len <= 2^27 elements as four base columns. */
int pw_stage_ext_to_cols(const uint32_t* d_in, size_t len, uint32_t* d_cols4);

/* The query pass of a STREAMED proof: rows idx[q] (q < n_idx <= 65535, HOST indices below 2 H) of the low-degree extension on the
 * 2 H = 2^(log_h + 1) points 31 w^j of `cols` polynomials given by their coefficient arrays as pw_lde_batch leaves them in d_coeffs
 * (bit-reversed, H-scaled, column stride H; 16-byte aligned): d_rows[q * cols + c], canonical Montgomery words (below p). The extended
 * domain is walked as 2^log_blocks sub-cosets (1 <= log_blocks <= min(5, log_h), log_h <= 26) of m = 2 H / 2^log_blocks rows; the
 * queries are bucketed by sub-coset and each sub-coset that holds one takes one of three forms, reported in forms[r] (may be NULL;
 * 2^log_blocks bytes; 0 = no query there):
 *   1  one pass, stored terms: the first stage group keeps every 2^12-row tile in LDS and stores the tile's term of each of the n_r
 *      queried rows; a second kernel sums a column's T = m / 2^12 tiles;
 *   2  one pass, 64-bit atomic sums in place of the stored terms;
 *   3  the partial transform (first stage group) of all cols columns into d_work, finished for the queried rows alone.
 * Forms 1 and 2 exist only where the sub-coset's transform has a first group of 12 stages on whole 2^12-row tiles and a second group
 * (m >= 2^14), log_blocks <= 2 and cols <= 65535. POWDR_QUERY_SELECT, read per call: 0 = always 3; 2 = 2 where it fits, else 3;
 * unset / 1 = 1 where it fits, else 2, else 3. With ev(x) = x rounded up to even, the one-pass forms need of d_work
 *   form 2:  A = 2^13 + ev(n_r) + ev(n_r T) + 2 cols n_r  words,        form 1:  A + cols T n_r  words,
 * and take the form only if that is at most select_words — the part of d_work OFFERED to them (a prover offers its whole sub-coset
 * buffer). d_work: 8-byte aligned, work_words >= cols m words (form 3's need; -1 below it, and for select_words > work_words).
 * d_scale: 2^13 words, as pw_lde_subcoset's. A d_coeffs that is not 16-byte aligned or a d_work that is not 8-byte aligned is refused
 * before any launch too, with hipErrorInvalidValue (as pw_lde_subcoset answers a misaligned d_coeffs). Owns the 2 n_idx words of its
 * bucketing tables and waits for the stream. */
int pw_stage_query_rows(const uint32_t* d_coeffs, uint32_t cols, uint32_t log_h, uint32_t log_blocks, const uint32_t* idx, uint32_t n_idx,
                        uint32_t* d_work, size_t work_words, size_t select_words, uint32_t* d_scale, uint32_t* d_rows, uint8_t* forms);

/* Host-side Poseidon2 permutation used by the transcript (canonical words in/out). This is also the known-answer-test
 * hook: after pw_set_poseidon2_constants a maintainer feeds it the vector of the backend's own Poseidon2 test. */
void pw_poseidon2_permute_host(uint32_t* state16);

/* The hash parameters are ONE table installed at run time. The shape is fixed (width 16, x^7, 4 + 13 + 4 rounds, external
 * layer circ(2 M4, M4, M4, M4) with M4 = [[2,3,1,1],[1,2,3,1],[1,1,2,3],[3,1,1,2]], internal layer 1 1^T + diag(-2, 1, 2,
 * 1/2, 3, 4, -1/2, -3, -4, 2^-8, 1/4, 1/8, 2^-27, -2^-8, -1/16, -2^-27) — the shape of p3-baby-bear's width-16 instance);
 * the ROUND CONSTANTS of the reference's permutation live in the un-vendored crate p3-baby-bear 0.5.2
 * (/root/reference/number/Cargo.toml:16-19: BABYBEAR_RC16_EXTERNAL_INITIAL / _FINAL / _INTERNAL), so the library starts with a
 * documented placeholder stream and takes the real table here: ext_rc = 8 x 16 canonical words (the four initial rounds,
 * then the four final ones), int_rc = 13 canonical words. Both NULL = back to the placeholder. Every derived table (folded
 * constants, per-stage scales of the device kernels) is rebuilt; host transcript, host verifiers and the device kernels of
 * every GPU use the new set from the next call on. Call it while no proof is in flight (the device copy is replaced after a
 * device-wide synchronisation); proofs made under different tables do not verify against each other. Returns 0, or -1 for a
 * word >= p / one NULL pointer. */
int pw_set_poseidon2_constants(const uint32_t* ext_rc, const uint32_t* int_rc);
/* The table in use (canonical words): 128 + 13 round constants and the 16 internal-diagonal entries; NULL = skip. */
void pw_get_poseidon2_constants(uint32_t* ext_rc, uint32_t* int_rc, uint32_t* diag);

#ifdef __cplusplus
}
#endif
#endif /* POWDR_PROVER_H */
