//! FFI declarations of libpowdr_gpu: one `extern "C"` block per header of `include/`, `#[repr(C)]` mirrors of their
//! structs. The first block IS `openvm/src/cuda_abi.rs:8-64` (same names, same argument order); the reference's
//! `#[repr(C)]` types (`cuda_abi.rs:66-95,149-169`) are re-exported from there when built inside the powdr workspace.
//! Kept in sync with the headers by tests/test_rust_adapter_sync.py (symbol sets and struct field order).
#![allow(non_camel_case_types, clippy::too_many_arguments)]

use core::ffi::{c_char, c_int, c_uint, c_void};

/// BabyBear in Montgomery form, the in-memory representation of `p3_baby_bear::BabyBear` (include/powdr_gpu.h `PowdrFp`).
pub type PowdrFp = u32;

// ---------------------------------------------------------------------------------------------- include/powdr_gpu.h
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct OriginalAir {
    pub width: i32,
    pub height: i32,
    pub buffer: *const PowdrFp,
    pub row_block_size: i32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct Subst {
    pub air_index: i32,
    pub col: i32,
    pub row: i32,
    pub apc_col: i32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct ExprSpan {
    pub off: u32,
    pub len: u32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct DerivedExprSpec {
    pub col_base: u64,
    pub span: ExprSpan,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct DevInteraction {
    pub bus_id: u32,
    pub num_args: u32,
    pub args_index_off: u32,
}

#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrCallMajorAir {
    pub buffer: *const PowdrFp,
    pub cells_per_call: i32,
    pub reserved: i32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrSubstCM {
    pub air_index: i32,
    pub slot: i32,
    pub apc_col: i32,
}

/// `POWDR_ORIG_*` (include/powdr_gpu.h): the thirteen instruction AIRs of openvm-riscv/tests/openvm_constraints.txt, keyed by the
/// short AIR name `OriginalAirs::opcode_to_air` resolves to
pub const POWDR_ORIG_KINDS: [&str; 13] = ["BaseAlu", "Shift", "LoadStore", "BranchEqual", "JalLui", "LessThan", "BranchLessThan", "Jalr",
                                          "LoadSignExtend", "DivRem", "MulH", "Multiplication", "Auipc"];
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrOrigInstr {
    pub kind: u32,
    pub opcode: u32,
    pub pc: u32,
    pub a: u32,
    pub b: u32,
    pub c: u32,
    pub e: u32,
    pub f: u32,
    pub g: u32,
    pub ts_delta: u32,
    pub air_row: u32,
    pub rec_off: u32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrRecordSubst {
    pub instr: i32,
    pub col: i32,
    pub apc_col: i32,
}

extern "C" {
    // ---- the reference ABI, openvm/src/cuda_abi.rs:8-64 ----
    pub fn _apc_tracegen(d_output: *mut PowdrFp, output_height: usize, d_original_airs: *const OriginalAir,
                         d_subs: *const Subst, n_subs: usize, num_apc_calls: i32) -> i32;
    pub fn _apc_apply_derived_expr(d_output: *mut PowdrFp, output_height: usize, num_apc_calls: i32,
                                   d_specs: *const DerivedExprSpec, n_cols: usize, d_bytecode: *const u32) -> i32;
    pub fn _apc_apply_bus(d_output: *const PowdrFp, num_apc_calls: i32, d_bytecode: *const u32, bytecode_len: usize,
                          d_interactions: *const DevInteraction, n_interactions: usize, d_arg_spans: *const ExprSpan,
                          n_arg_spans: usize, var_range_bus_id: u32, d_var_hist: *mut u32, var_num_bins: usize,
                          tuple2_bus_id: u32, d_tuple2_hist: *mut u32, tuple2_sz0: u32, tuple2_sz1: u32,
                          bitwise_bus_id: u32, d_bitwise_hist: *mut u32) -> i32;
    // ---- extensions ----
    pub fn powdr_apc_apply_derived_expr_cols(d_output: *mut PowdrFp, output_height: usize, num_apc_calls: i32,
                                             d_specs: *const DerivedExprSpec, n_cols: usize, d_bytecode: *const u32) -> i32;
    pub fn powdr_apc_apply_bus_cols(d_output: *const PowdrFp, output_height: usize, num_apc_calls: i32,
                                    d_bytecode: *const u32, bytecode_len: usize, d_interactions: *const DevInteraction,
                                    n_interactions: usize, d_arg_spans: *const ExprSpan, n_arg_spans: usize,
                                    var_range_bus_id: u32, d_var_hist: *mut u32, var_num_bins: usize, tuple2_bus_id: u32,
                                    d_tuple2_hist: *mut u32, tuple2_sz0: u32, tuple2_sz1: u32, bitwise_bus_id: u32,
                                    d_bitwise_hist: *mut u32) -> i32;
    pub fn powdr_apc_tracegen_host_tables(d_output: *mut PowdrFp, output_height: usize, d_original_airs: *const OriginalAir,
                                          h_original_airs: *const OriginalAir, n_airs: usize, h_subs: *const Subst,
                                          n_subs: usize, num_apc_calls: i32) -> i32;
    pub fn powdr_apc_apply_bus_host_tables(d_output: *const PowdrFp, output_height: usize, num_apc_calls: i32,
                                           d_bytecode: *const u32, h_bytecode: *const u32, bytecode_len: usize,
                                           d_interactions: *const DevInteraction, h_interactions: *const DevInteraction,
                                           n_interactions: usize, d_arg_spans: *const ExprSpan, h_arg_spans: *const ExprSpan,
                                           n_arg_spans: usize, var_range_bus_id: u32, d_var_hist: *mut u32,
                                           var_num_bins: usize, tuple2_bus_id: u32, d_tuple2_hist: *mut u32,
                                           tuple2_sz0: u32, tuple2_sz1: u32, bitwise_bus_id: u32,
                                           d_bitwise_hist: *mut u32) -> i32;
    pub fn powdr_apc_tracegen_callmajor(d_output: *mut PowdrFp, output_height: usize, h_airs: *const PowdrCallMajorAir, n_airs: usize,
                                        h_subs: *const PowdrSubstCM, n_subs: usize, num_apc_calls: i32) -> i32;
    pub fn powdr_original_airs_expand(d_records: *const u32, num_calls: usize, h_instrs: *const PowdrOrigInstr, n_instrs: usize,
                                      h_airs: *const OriginalAir) -> i32;
    pub fn powdr_apc_tracegen_records(d_output: *mut PowdrFp, output_height: usize, d_records: *const u32, num_apc_calls: usize,
                                      h_instrs: *const PowdrOrigInstr, n_instrs: usize, h_subs: *const PowdrRecordSubst, n_subs: usize) -> i32;
    pub fn powdr_original_row_expand_host(instr: *const PowdrOrigInstr, record_words6: *const u32, timestamp: u32, row_out: *mut u32) -> i32;
    pub fn powdr_periphery_var_range_trace(d_var_hist: *const u32, var_num_bins: usize, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_tuple2_trace(d_tuple2_hist: *const u32, tuple2_sz0: u32, tuple2_sz1: u32, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_bitwise_trace(d_bitwise_hist: *const u32, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_var_range_table(var_num_bins: usize, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_tuple2_table(tuple2_sz0: u32, tuple2_sz1: u32, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_bitwise_table(d_out: *mut PowdrFp) -> i32;
    pub fn powdr_periphery_multiplicities(d_hist: *const u32, n: usize, d_out: *mut PowdrFp) -> i32;
    pub fn powdr_gpu_set_stream(hip_stream: *mut c_void);
    pub fn powdr_gpu_get_stream() -> *mut c_void;
    pub fn powdr_gpu_timing_enable(enable: c_int);
    pub fn powdr_gpu_timing_report(buf: *mut c_char, cap: usize) -> usize;
    pub fn powdr_gpu_call_stats(out16: *mut u64, reset: c_int);
    pub fn powdr_gpu_version() -> *const c_char;
}

// --------------------------------------------------------------------------------------------- include/powdr_host.h
#[repr(C)]
pub struct PowdrApc {
    _opaque: [u8; 0],
}
#[repr(C)]
pub struct PowdrApcCandidates {
    _opaque: [u8; 0],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrDeviceMatrix {
    pub buffer: *const PowdrFp,
    pub width: i32,
    pub height: i32,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PowdrPeriphery {
    pub var_range_bus_id: u32,
    pub d_var_hist: *mut u32,
    pub var_num_bins: usize,
    pub tuple2_bus_id: u32,
    pub d_tuple2_hist: *mut u32,
    pub tuple2_sz0: u32,
    pub tuple2_sz1: u32,
    pub bitwise_bus_id: u32,
    pub d_bitwise_hist: *mut u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PowdrAirStats {
    pub main_columns: u64,
    pub constraints: u64,
    pub bus_interactions: u64,
}
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PowdrApcCandidateInfo {
    pub execution_frequency: u64,
    pub start_pc: u64,
    pub n_blocks: u32,
    pub n_instructions: u32,
    pub before: PowdrAirStats,
    pub after: PowdrAirStats,
    pub width_before: u64,
    pub value: u64,
    pub cost_before: f64,
    pub cost_after: f64,
}

extern "C" {
    pub fn powdr_apc_from_json(json: *const c_char, len: usize, err: *mut c_char, err_cap: usize) -> *mut PowdrApc;
    pub fn powdr_apc_from_json_at(json: *const c_char, len: usize, index: usize, err: *mut c_char, err_cap: usize) -> *mut PowdrApc;
    pub fn powdr_apc_count_in_json(json: *const c_char, len: usize) -> usize;
    pub fn powdr_apc_from_cbor(bytes: *const u8, len: usize, index: usize, err: *mut c_char, err_cap: usize) -> *mut PowdrApc;
    pub fn powdr_apc_count_in_cbor(bytes: *const u8, len: usize) -> usize;
    pub fn powdr_apc_free(apc: *mut PowdrApc);
    pub fn powdr_apc_width(apc: *const PowdrApc) -> u32;
    pub fn powdr_apc_poly_ids(apc: *const PowdrApc) -> *const u64;
    pub fn powdr_apc_num_constraints(apc: *const PowdrApc) -> u32;
    pub fn powdr_apc_num_bus_interactions(apc: *const PowdrApc) -> u32;
    pub fn powdr_apc_num_derived_columns(apc: *const PowdrApc) -> u32;
    pub fn powdr_apc_num_instructions(apc: *const PowdrApc) -> u32;
    pub fn powdr_apc_instruction_opcode(apc: *const PowdrApc, i: u32) -> u32;
    pub fn powdr_apc_instruction_num_subs(apc: *const PowdrApc, i: u32) -> u32;
    pub fn powdr_apc_bus_map_len(apc: *const PowdrApc) -> usize;
    pub fn powdr_apc_bus_map_entry(apc: *const PowdrApc, i: usize, bus_id: *mut u64, kind: *mut u32, sizes2: *mut u32,
                                   name: *mut c_char, name_cap: usize) -> c_int;
    pub fn powdr_apc_periphery_from_bus_map(apc: *const PowdrApc, periphery: *mut PowdrPeriphery) -> c_int;
    pub fn powdr_apc_candidates_from_json(json: *const c_char, len: usize, err: *mut c_char, err_cap: usize) -> *mut PowdrApcCandidates;
    pub fn powdr_apc_candidates_free(c: *mut PowdrApcCandidates);
    pub fn powdr_apc_candidates_version(c: *const PowdrApcCandidates) -> u64;
    pub fn powdr_apc_candidates_count(c: *const PowdrApcCandidates) -> usize;
    pub fn powdr_apc_candidates_num_labels(c: *const PowdrApcCandidates) -> usize;
    pub fn powdr_apc_candidates_get(c: *const PowdrApcCandidates, i: usize, out: *mut PowdrApcCandidateInfo) -> c_int;
    pub fn powdr_apc_compile_bus(apc: *const PowdrApc, apc_height: usize, interactions: *mut DevInteraction,
                                 arg_spans: *mut ExprSpan, n_arg_spans: *mut usize, bytecode: *mut u32) -> usize;
    pub fn powdr_apc_compile_derived(apc: *const PowdrApc, apc_height: usize, specs: *mut DerivedExprSpec, bytecode: *mut u32) -> usize;
    pub fn powdr_apc_compile_constraints(apc: *const PowdrApc, spans: *mut ExprSpan, bytecode: *mut u32) -> usize;
    pub fn powdr_apc_build_substitutions(apc: *const PowdrApc, instr_air: *const i32, subs: *mut Subst, air_ids_out: *mut i32,
                                         row_block_out: *mut i32, n_airs: *mut usize) -> usize;
    pub fn powdr_apc_generate_witness_gpu(apc: *mut PowdrApc, instr_air: *const i32, dummy_by_air: *const PowdrDeviceMatrix,
                                          n_dummy: usize, num_apc_calls: usize, d_output: *mut PowdrFp,
                                          periphery: *const PowdrPeriphery) -> c_int;
    pub fn powdr_apc_instruction_table(apc: *const PowdrApc, out: *mut PowdrOrigInstr, words_per_call: *mut usize) -> usize;
    pub fn powdr_apc_generate_witness_from_records(apc: *mut PowdrApc, d_records: *const u32, num_apc_calls: usize, d_output: *mut PowdrFp,
                                                   periphery: *const PowdrPeriphery) -> c_int;
    pub fn powdr_xbc_eval_host(postfix: *const u32, len: u32, trace: *const u32, r: usize, result: *mut u32, n_instr: *mut u32) -> c_int;
    pub fn powdr_small_form_eval_host(postfix: *const u32, len: u32, trace: *const u32, r: usize, result: *mut u32, flags: *mut u32) -> c_int;
    pub fn powdr_field_selftest(seed: u64, iterations: u32) -> c_int;
    pub fn powdr_field_selftest_gpu(seed: u64, iterations: u32, failing_check: *mut c_int) -> c_int;
    pub fn powdr_poseidon2_derived(out: *mut i64, cap: usize) -> usize;
}

// ------------------------------------------------------------------------------------------- include/powdr_prover.h
/// `PwSegmentProveFn` of include/powdr_prover.h: one worker's replica of the per-segment pipeline.
pub type PwSegmentProveFn = unsafe extern "C" fn(user: *mut c_void, segment: usize, worker: usize, device: c_int, commitment8: *mut u32) -> c_int;

#[repr(C)]
pub struct PwProver {
    _opaque: [u8; 0],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwStarkConfig {
    pub num_queries: u32,
    pub pow_bits: u32,
}
/// One matrix of `pw_stage_gather_rows_multi`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwStageGatherJob {
    pub d_m: *const u32,
    pub height: u64,
    pub width: u32,
    pub idx_off: u32,
    pub out_off: u64,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwSegmentAir {
    pub prover: *mut PwProver,
    pub d_trace: *const u32,
    pub log_height: u32,
    /// read by `pw_prove_segment_consuming` only (`PW_AIR_HAND_OVER`)
    pub flags: u32,
}
/// `PwSegmentAir::flags`: the trace is the engine's to overwrite
pub const PW_AIR_HAND_OVER: u32 = 1;
/// `PwBusTuple::args` holds the first 16 words of a tuple
pub const PW_BUS_MAX_ARGS: usize = 16;
/// `pw_check_segment_buses` flags: run the tuple tally for balanced buses too
pub const PW_BUS_CHECK_TALLY_ALL: u32 = 1;
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwBusSummary {
    pub bus: u32,
    /// 0 balanced; 1 unbalanced, tuples listed; 2 unbalanced, tally table too small: not localised
    pub status: u32,
    pub n_active: u64,
    pub n_unbalanced: u64,
}
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwBusTuple {
    pub bus: u32,
    pub n_args: u32,
    pub args: [u32; PW_BUS_MAX_ARGS],
    pub net_multiplicity: u32,
    pub air: u32,
    pub interaction: u32,
    pub row: u64,
    pub n_contributions: u64,
}
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwSystemTraceStats {
    pub table_slots: u64,
    pub occupied_slots: u64,
    pub tables: u64,
    pub walked: u64,
    pub additions: u64,
    pub lds_atomics: u64,
    pub global_atomics: u64,
}
/// a basic block of `pw_empirical_detect`: `n_instructions` instructions from `start_pc` on, `pc_step` apart
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwBasicBlock {
    pub start_pc: u32,
    pub n_instructions: u32,
}
/// the opaque host-side result of `pw_empirical_detect`
#[repr(C)]
pub struct PwEmpirical {
    _private: [u8; 0],
}
/// the opaque result of `pw_execution_blocks_from_*`: host-side tables and the head sequence kept on the device
#[repr(C)]
pub struct PwExecutionBlocks {
    _private: [u8; 0],
}
/// an operand of an optimistic constraint: kind 0 `Number(value)`, 1 `Pc(instr_idx)`, 2 `RegisterLimb(instr_idx, reg, limb)`
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwApcOperand {
    pub kind: u32,
    pub instr_idx: u32,
    pub reg: u32,
    pub limb: u32,
    pub value: u64,
}
/// an optimistic constraint `left == right`
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwApcConstraint {
    pub left: PwApcOperand,
    pub right: PwApcOperand,
}
/// an APC of `pw_apc_calls_from_*`: its constraints are `[first_constraint, first_constraint + n_constraints)` of the flat array
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwApc {
    pub start_pc: u32,
    pub cycle_count: u32,
    pub priority: u64,
    pub first_constraint: u64,
    pub n_constraints: u64,
}
/// the opaque host-side result of `pw_apc_calls_from_*`
#[repr(C)]
pub struct PwApcCalls {
    _private: [u8; 0],
}
/// the opaque result of `pw_apc_sources_from_traces`: source and residual matrices on the device
#[repr(C)]
pub struct PwApcSources {
    _private: [u8; 0],
}
/// a job of `pw_trace_gather_rows`: `out[c * h_out + i] = in[c * h_in + idx[i]]`, `idx[i] == !0` = a zero row (device pointers)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PwGatherJob {
    pub r#in: *const u32,
    pub h_in: u64,
    pub width: u64,
    pub idx: *const u32,
    pub out: *mut u32,
    pub h_out: u64,
}
/// `flags` of `pw_apc_sources_from_traces_flags`: keep the index lists, build no source matrices
pub const PW_APC_SOURCES_DIRECT: u32 = 1;
/// a cell of `pw_apc_sources_tracegen`: column `col` of the AIR of the APC's instruction `instr` feeds APC column `apc_col`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PwApcCell {
    pub instr: u32,
    pub col: u32,
    pub apc_col: u32,
}
/// a job of `pw_apc_sources_tracegen`: the named columns of one APC's trace (`cells` on the host, `d_out` on the device)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PwApcTraceJob {
    pub apc: u32,
    pub cells: *const PwApcCell,
    pub n_cells: usize,
    pub d_out: *mut u32,
    pub out_height: u64,
    pub out_width: u32,
}
/// the limits of `pw_execution_segments_from_traces`: a class holds at most `2^max_log_height` rows, heights are padded to at least
/// `2^min_log_height`, `max_cells` bounds the sum of width x padded height (0 = no bound), `max_segments` 0 = 2^20
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PwSegmentLimits {
    pub max_log_height: u32,
    pub min_log_height: u32,
    pub max_cells: u64,
    pub max_segments: u64,
}
/// what `pw_execution_segments_from_traces_metered` meters: the memory bus, the memory tree's height (1 .. 30), and per
/// system AIR (0 = boundary, 1 = memory Merkle, 2 = the Poseidon2 bound 2 M) its log2 cap and the width it counts with under `max_cells`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct PwSystemMeter {
    pub memory_bus: u32,
    pub tree_height: u32,
    pub max_log_height: [u32; 3],
    pub width: [u32; 3],
}
/// the opaque result of `pw_execution_segments_from_traces`: the cuts on the host, the per-(segment, AIR) row lists on the device
#[repr(C)]
pub struct PwExecutionSegments {
    _private: [u8; 0],
}
/// the opaque result of `pw_execution_states_from_traces`: the states of a segment on the device
#[repr(C)]
pub struct PwExecutionStates {
    _private: [u8; 0],
}
/// `pw_memory_tree_set_mode`: every level above level 0 hashed again from the level below
pub const PW_MEMORY_TREE_REBUILD: u32 = 0;
/// `pw_memory_tree_set_mode`: only the touched paths hashed, every other stored node moved
pub const PW_MEMORY_TREE_INCREMENTAL: u32 = 1;
/// the opaque handle of `pw_memory_tree_create`
#[repr(C)]
pub struct PwMemoryTree {
    _private: [u8; 0],
}
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwMemoryTreeStats {
    pub leaves: u64,
    pub stored_nodes: u64,
    pub device_bytes: u64,
    pub last_permutations: u64,
    pub last_launches: u64,
    pub last_scratch_bytes: u64,
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwAirDescription {
    pub width: u32,
    pub log_height: u32,
    pub logup: u32,
    pub cons_bytecode: *const u32,
    pub bytecode_len: usize,
    pub cons_spans: *const u32,
    pub n_constraints: usize,
    pub interactions: *const u32,
    pub n_interactions: usize,
    pub inter_spans: *const u32,
    pub n_inter_spans: usize,
    pub inter_bytecode: *const u32,
    pub inter_bytecode_len: usize,
}
/// The verifying key's part of an AIR with preprocessed columns (`width` 0: none); `root8` = `pw_prover_preprocessed_root`
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwAirPreprocessed {
    pub width: u32,
    pub root8: [u32; 8],
}
/// The public values of one AIR as the verifier is told them: `n` of them, `expected` null = accept the proof's
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwAirPublic {
    pub n: u32,
    pub expected: *const u32,
}
/// One segment of `pw_verify_segment_chain`
#[repr(C)]
#[derive(Clone, Copy)]
pub struct PwChainSegment {
    pub airs: *const PwAirDescription,
    pub pre: *const PwAirPreprocessed,
    pub pub_: *const PwAirPublic,
    pub n_airs: usize,
    pub logup: c_int,
    pub proof: *const u32,
    pub n_words: usize,
    pub check_balance: c_int,
}
/// public value `index_from` of AIR `air_from` in segment s = public value `index_to` of AIR `air_to` in segment s + 1
#[repr(C)]
#[derive(Clone, Copy, Default, Debug)]
pub struct PwChainLink {
    pub air_from: u32,
    pub index_from: u32,
    pub air_to: u32,
    pub index_to: u32,
}

extern "C" {
    pub fn pw_prover_create(cfg: *const PwStarkConfig, width: u32, cons_bytecode: *const u32, bytecode_len: usize,
                            cons_spans: *const u32, n_constraints: usize) -> *mut PwProver;
    pub fn pw_prover_create_logup(cfg: *const PwStarkConfig, width: u32, cons_bytecode: *const u32, bytecode_len: usize,
                                  cons_spans: *const u32, n_constraints: usize, interactions: *const u32,
                                  n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                  inter_bytecode: *const u32, inter_bytecode_len: usize) -> *mut PwProver;
    pub fn pw_prover_trace_root(p: *mut PwProver, d_trace: *const u32, log_height: u32, root8: *mut u32) -> c_int;
    pub fn pw_prover_set_bus_seed(p: *mut PwProver, seed8: *const u32) -> c_int;
    pub fn pw_prover_logup_path(p: *const PwProver) -> c_int;
    pub fn pw_prover_destroy(p: *mut PwProver);
    pub fn pw_prover_create_preprocessed(cfg: *const PwStarkConfig, width: u32, pre_width: u32, log_height: u32, d_pre: *const u32,
                                         cons_bytecode: *const u32, bytecode_len: usize, cons_spans: *const u32, n_constraints: usize,
                                         interactions: *const u32, n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                         inter_bytecode: *const u32, inter_bytecode_len: usize) -> *mut PwProver;
    pub fn pw_prover_preprocessed_root(p: *const PwProver, root8: *mut u32) -> c_int;
    pub fn pw_prover_preprocessed_width(p: *const PwProver) -> u32;
    /// next-row operands and row selectors in the constraints: operands W1..2W1 = the next row, 2W1..2W1+3 =
    /// is_first_row / is_last_row / is_transition (W1 = width + pre_width); pre_width = 0: no fixed matrix; segment proofs only
    pub fn pw_prover_create_transition(cfg: *const PwStarkConfig, width: u32, pre_width: u32, log_height: u32, d_pre: *const u32,
                                       cons_bytecode: *const u32, bytecode_len: usize, cons_spans: *const u32, n_constraints: usize,
                                       interactions: *const u32, n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                       inter_bytecode: *const u32, inter_bytecode_len: usize) -> *mut PwProver;
    /// bit 0: reads a next-row operand, bit 1: reads a selector (0: not row-aware)
    pub fn pw_prover_row_flags(p: *const PwProver) -> u32;
    /// public values: constraint operands 2 W1 + 3 + k, k < n_public <= 256, degree 0; n_public = 0: exactly
    /// `pw_prover_create_transition`; segment proofs only, after `pw_prover_set_public_values`
    pub fn pw_prover_create_public(cfg: *const PwStarkConfig, width: u32, pre_width: u32, log_height: u32, d_pre: *const u32, n_public: u32,
                                   cons_bytecode: *const u32, bytecode_len: usize, cons_spans: *const u32, n_constraints: usize,
                                   interactions: *const u32, n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                   inter_bytecode: *const u32, inter_bytecode_len: usize) -> *mut PwProver;
    pub fn pw_prover_n_public(p: *const PwProver) -> u32;
    /// `values`: n canonical host words (copied); -1: n != n_public or a word >= p
    pub fn pw_prover_set_public_values(p: *mut PwProver, values: *const u32, n: usize) -> c_int;
    pub fn pw_prover_prove(p: *mut PwProver, d_trace: *const u32, log_height: u32, proof_words: *mut *const u32,
                           n_words: *mut usize) -> c_int;
    /// The trace is handed over (the engine owns `common_main`): a streamed proof leaves the coefficient arrays in its place.
    pub fn pw_prover_prove_consuming(p: *mut PwProver, d_trace: *mut u32, log_height: u32, proof_words: *mut *const u32,
                                     n_words: *mut usize) -> c_int;
    pub fn pw_prover_stream_log_blocks_consuming(p: *const PwProver, log_height: u32) -> c_int;
    pub fn pw_trace_from_coefficients(d_coeffs: *mut u32, width: u32, log_height: u32, d_scratch: *mut u32) -> c_int;
    pub fn pw_prover_check_constraints(p: *mut PwProver, d_trace: *const u32, log_height: u32, n_violations: *mut u64,
                                       first_row: *mut u64, first_constraint: *mut u32) -> c_int;
    /// the bus half of the mock prover (`debug_proving_ctx`): per bus balanced or not, and the unbalanced tuples with a witness each
    pub fn pw_check_segment_buses(airs: *const PwSegmentAir, n_airs: usize, buses: *const u32, n_buses: usize, seed: u64,
                                  table_bytes: usize, flags: u32, summaries: *mut PwBusSummary, summary_cap: usize,
                                  n_summaries: *mut usize, tuples: *mut PwBusTuple, tuple_cap: usize, n_tuples: *mut usize) -> c_int;
    pub fn pw_bus_check_scratch_bytes() -> usize;
    pub fn pw_bus_check_peak_bytes() -> usize;
    /// The program AIR's multiplicity column from what the other AIRs send on the PC-lookup bus; tuples that equal no table row are counted.
    pub fn pw_program_frequencies(airs: *const PwSegmentAir, n_airs: usize, bus: u32, pc_base: u32, pc_step: u32, d_program: *const u32,
                                  log_h: u32, d_freq_out: *mut u32, n_foreign: *mut u64, first_foreign: *mut PwBusTuple) -> c_int;
    /// The memory boundary AIR's trace (18 columns, one row per touched location, sorted) from the memory bus; `status` 0 = written.
    pub fn pw_memory_boundary_trace(airs: *const PwSegmentAir, n_airs: usize, bus: u32, table_bytes: usize, d_trace_out: *mut u32,
                                    cap_log_height: u32, log_height: *mut u32, n_locations: *mut u64, status: *mut u32) -> c_int;
    pub fn pw_system_traces_scratch_bytes() -> usize;
    pub fn pw_system_traces_peak_bytes() -> usize;
    pub fn pw_system_traces_last_stats(out: *mut PwSystemTraceStats);
    /// 2^log_slots slots in the first address table of this thread's later `pw_memory_boundary_trace` calls (0 = default)
    pub fn pw_memory_boundary_set_start_slots(log_slots: u32) -> c_int;
    /// the Poseidon2 compression chip's trace from the senders on `bus` (status 1: retry with `cap_log_height = *log_height`)
    pub fn pw_poseidon2_compress_trace(airs: *const PwSegmentAir, n_airs: usize, bus: u32, table_bytes: usize, start_log_slots: u32,
                                       d_trace_out: *mut u32, cap_log_height: u32, log_height: *mut u32, n_rows: *mut u64,
                                       status: *mut u32) -> c_int;
    /// Empirical constraints: per pc the percentile range of every column, per listed block its classes of equal cells.
    /// `status` 0 = `*out` is set (free it with `pw_empirical_destroy`); otherwise no result and `info` says where.
    pub fn pw_empirical_detect(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bus: u32, pc_step: u32,
                               blocks: *const PwBasicBlock, n_blocks: usize, scratch_bytes: usize, out: *mut *mut PwEmpirical,
                               status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_empirical_destroy(e: *mut PwEmpirical);
    /// sizes[5] = pcs, ranges, blocks that ran, classes, cells
    pub fn pw_empirical_sizes(e: *const PwEmpirical, sizes: *mut u64);
    pub fn pw_empirical_read_pcs(e: *const PwEmpirical, pcs: *mut u32, counts: *mut u64, air_of_pc: *mut u32, range_offsets: *mut u64);
    pub fn pw_empirical_read_ranges(e: *const PwEmpirical, lo_hi: *mut u32);
    pub fn pw_empirical_read_blocks(e: *const PwEmpirical, start_pcs: *mut u32, class_offsets: *mut u64, cell_offsets: *mut u64);
    pub fn pw_empirical_read_cells(e: *const PwEmpirical, instruction_column: *mut u32);
    /// n / 100 and n * 99 / 100: host only
    pub fn pw_empirical_percentile_indices(n: u64, lo: *mut u64, hi: *mut u64);
    /// a test hook: ANDed onto both fingerprint halves of this thread's later `pw_empirical_detect` calls (0 = full width)
    pub fn pw_empirical_set_fingerprint_mask(mask: u64);
    /// out[6]: panels, seeds, active rows, cells verified, peak scratch bytes, scratch bytes held
    pub fn pw_empirical_last_stats(out: *mut u64);
    /// Superblock detection: pc counts, distinct basic-block runs and the greedy counts of every window of up to
    /// `max_bb` blocks, from the execution's pcs on the device. `status` 0 = `*out` is set (free it with `pw_execution_blocks_destroy`).
    pub fn pw_execution_blocks_from_pcs(d_pcs: *const u32, n: u64, pc_step: u32, blocks: *const PwBasicBlock, n_blocks: usize, max_bb: u32,
                                        scratch_bytes: usize, out: *mut *mut PwExecutionBlocks, status: *mut u32, info: *mut u64) -> c_int;
    /// the same from the instruction AIRs' traces, read as `pw_empirical_detect` reads them
    pub fn pw_execution_blocks_from_traces(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bus: u32, pc_step: u32,
                                           blocks: *const PwBasicBlock, n_blocks: usize, max_bb: u32, scratch_bytes: usize,
                                           out: *mut *mut PwExecutionBlocks, status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_execution_blocks_destroy(e: *mut PwExecutionBlocks);
    /// sizes[6] = pcs, runs, start pcs of all runs, superblocks, start pcs of all superblocks, heads kept on the device
    pub fn pw_execution_blocks_sizes(e: *const PwExecutionBlocks, sizes: *mut u64);
    pub fn pw_execution_blocks_read_pc_counts(e: *const PwExecutionBlocks, pcs: *mut u32, counts: *mut u64);
    pub fn pw_execution_blocks_read_runs(e: *const PwExecutionBlocks, offsets: *mut u64, start_pcs: *mut u32, counts: *mut u64);
    pub fn pw_execution_blocks_read_superblocks(e: *const PwExecutionBlocks, offsets: *mut u64, start_pcs: *mut u32, counts: *mut u64);
    /// the greedy non-overlapping occurrences of a candidate over what is left of the execution; `remove` takes them out
    pub fn pw_execution_blocks_count(e: *mut PwExecutionBlocks, needle_start_pcs: *const u32, len: u32, remove: c_int, count: *mut u64) -> c_int;
    /// a test hook: ANDed onto both fingerprint halves of this thread's later `pw_execution_blocks_from_*` calls (0 = full width)
    pub fn pw_execution_blocks_set_fingerprint_mask(mask: u64);
    /// out[7]: levels, clusters counted by pointer doubling, seeds, heads, runs, peak scratch bytes, scratch bytes held
    pub fn pw_execution_blocks_last_stats(out: *mut u64);
    /// APC call selection: the calls the reference's `ApcCandidates` extracts, from the execution's states on the
    /// device. `status` 0 = `*out` is set (free it with `pw_apc_calls_destroy`).
    pub fn pw_apc_calls_from_states(d_pcs: *const u32, d_regs: *const u32, n_states: u64, n_regs: u32, limb_bits: u32, apcs: *const PwApc, n_apcs: usize,
                                    constraints: *const PwApcConstraint, n_constraints: usize, scratch_bytes: usize, out: *mut *mut PwApcCalls,
                                    status: *mut u32, info: *mut u64) -> c_int;
    /// the same from the instruction AIRs' traces of ONE segment (pcs only); `final_pc` = the pc after the last row
    pub fn pw_apc_calls_from_traces(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bus: u32, final_pc: u32, apcs: *const PwApc,
                                    n_apcs: usize, constraints: *const PwApcConstraint, n_constraints: usize, scratch_bytes: usize,
                                    out: *mut *mut PwApcCalls, status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_apc_calls_destroy(e: *mut PwApcCalls);
    /// sizes[5] = calls, APCs, positions covered by calls, states, time keys
    pub fn pw_apc_calls_sizes(e: *const PwApcCalls, sizes: *mut u64);
    pub fn pw_apc_calls_read_calls(e: *const PwApcCalls, apc_ids: *mut u32, from: *mut u64, to: *mut u64);
    /// 7 per APC: matches, refused, failed, aborted, done, discarded, calls
    pub fn pw_apc_calls_read_counters(e: *const PwApcCalls, counters: *mut u64);
    pub fn pw_apc_calls_read_time_keys(e: *const PwApcCalls, keys: *mut u64);
    /// a test hook: components of more than `n` candidates take the fold's long path in this thread's later calls (0 = the default)
    pub fn pw_apc_calls_set_long_threshold(n: u64);
    /// out[7]: candidates, valid, components, longest component, components on the long path, peak scratch bytes, scratch bytes held
    pub fn pw_apc_calls_last_stats(out: *mut u64);
    /// the states of ONE segment from its traces: pcs, the registers `regs` read off the memory bus and the time
    /// keys, kept on the device in the layout `pw_apc_calls_from_states` reads. `status` 0 = `*out` is set (free it with
    /// `pw_execution_states_destroy`); 8 = a register tuple that is none, 9 = a register without a value, 10 = `initial_regs` contradicted
    pub fn pw_execution_states_from_traces(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, memory_bus: u32,
                                           final_pc: u32, reg_as: u32, reg_ptr_step: u32, regs: *const u32, n_regs: usize, initial_regs: *const u32,
                                           scratch_bytes: usize, out: *mut *mut PwExecutionStates, status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_execution_states_destroy(e: *mut PwExecutionStates);
    /// sizes[4] = states, registers, register sends read, device bytes held
    pub fn pw_execution_states_sizes(e: *const PwExecutionStates, sizes: *mut u64);
    pub fn pw_execution_states_device(e: *const PwExecutionStates, d_pcs: *mut *const u32, d_regs: *mut *const u32, d_time_keys: *mut *const u64);
    pub fn pw_execution_states_read(e: *const PwExecutionStates, pcs: *mut u32, regs: *mut u32, time_keys: *mut u64) -> c_int;
    /// out[5]: register sends read, sends kept, the fill's tile in table words, peak scratch bytes, scratch bytes held
    pub fn pw_execution_states_last_stats(out: *mut u64);
    /// `pw_apc_calls_from_traces` with `RegisterLimb` operands: the registers the constraints name come from the memory bus
    pub fn pw_apc_calls_from_traces_registers(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, memory_bus: u32,
                                              final_pc: u32, reg_as: u32, reg_ptr_step: u32, n_regs: u32, limb_bits: u32, initial_regs: *const u32,
                                              apcs: *const PwApc, n_apcs: usize, constraints: *const PwApcConstraint, n_constraints: usize,
                                              scratch_bytes: usize, out: *mut *mut PwApcCalls, status: *mut u32, info: *mut u64) -> c_int;
    /// the row gather of DESIGN.md §5t on caller-owned device buffers, all jobs in one launch
    pub fn pw_trace_gather_rows(jobs: *const PwGatherJob, n_jobs: usize) -> c_int;
    /// applying the calls of ONE segment: per (APC, AIR) the call-major source matrix `_apc_tracegen` reads, per AIR
    /// the residual trace. `status` 0 = `*out` is set (free it with `pw_apc_sources_destroy`); 11 = a call beyond the execution,
    /// 12 = two calls of one APC disagree on an instruction's AIR
    pub fn pw_apc_sources_from_traces(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, cycle_counts: *const u32,
                                      n_apcs: usize, call_apc_ids: *const u32, call_from: *const u64, call_to: *const u64, n_calls: usize,
                                      min_log_height: u32, scratch_bytes: usize, out: *mut *mut PwApcSources, status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_apc_sources_destroy(e: *mut PwApcSources);
    /// sizes[6] = APCs, AIRs, positions, covered positions, source bytes, residual bytes
    pub fn pw_apc_sources_sizes(e: *const PwApcSources, sizes: *mut u64);
    pub fn pw_apc_sources_layout(e: *const PwApcSources, apc: u32, n_calls: *mut u64, air: *mut u32, occ: *mut u32) -> i64;
    pub fn pw_apc_sources_source(e: *const PwApcSources, apc: u32, air: u32, d_matrix: *mut *const u32, width: *mut u32, height: *mut u64,
                                 row_block_size: *mut u32) -> c_int;
    pub fn pw_apc_sources_residual(e: *const PwApcSources, air: u32, d_matrix: *mut *const u32, rows: *mut u64, log_height: *mut u32) -> c_int;
    pub fn pw_apc_sources_read_source(e: *const PwApcSources, apc: u32, air: u32, words: *mut u32) -> c_int;
    pub fn pw_apc_sources_read_residual(e: *const PwApcSources, air: u32, words: *mut u32) -> c_int;
    /// out[8]: covered positions, source bytes, residual bytes, gather jobs, 16-byte-load tiles, 4-byte-load tiles, peak scratch, scratch held
    pub fn pw_apc_sources_last_stats(out: *mut u64);
    /// `pw_apc_sources_from_traces` with `flags`: 0 = the same call; `PW_APC_SOURCES_DIRECT` = no source matrices, the handle keeps the
    /// index lists and the AIRs' trace pointers — the traces must outlive the last `pw_apc_sources_tracegen`
    pub fn pw_apc_sources_from_traces_flags(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, cycle_counts: *const u32,
                                            n_apcs: usize, call_apc_ids: *const u32, call_from: *const u64, call_to: *const u64, n_calls: usize,
                                            min_log_height: u32, scratch_bytes: usize, flags: u32, out: *mut *mut PwApcSources, status: *mut u32,
                                            info: *mut u64) -> c_int;
    /// the bytes of a direct handle's index lists (0 on a flags-0 handle)
    pub fn pw_apc_sources_index_bytes(e: *const PwApcSources) -> u64;
    /// the named columns of the APC traces straight from the chips' traces, all jobs in one launch; -1 = malformed, or no direct handle
    pub fn pw_apc_sources_tracegen(e: *const PwApcSources, jobs: *const PwApcTraceJob, n_jobs: usize) -> c_int;
    /// out[6]: jobs, work items, 16-byte-load tiles, 4-byte-load tiles, bytes written, scratch held
    pub fn pw_apc_sources_tracegen_last_stats(out: *mut u64);
    /// cutting ONE execution into segments under APC-aware limits: the greedy cut that never falls inside a call.
    /// `status` 0 = `*out` is set (free it with `pw_execution_segments_destroy`); 11 = a call beyond the execution, 13 = nothing
    /// fits under `max_cells`, 14 = more than `max_segments` segments
    pub fn pw_execution_segments_from_traces(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, final_pc: u32,
                                             cycle_counts: *const u32, apc_widths: *const u32, n_apcs: usize, call_apc_ids: *const u32,
                                             call_from: *const u64, call_to: *const u64, n_calls: usize, limits: *const PwSegmentLimits,
                                             scratch_bytes: usize, out: *mut *mut PwExecutionSegments, status: *mut u32, info: *mut u64) -> c_int;
    pub fn pw_execution_segments_destroy(e: *mut PwExecutionSegments);
    /// sizes[6] = segments, AIRs, APCs, positions, covered positions, bytes of the row lists
    pub fn pw_execution_segments_sizes(e: *const PwExecutionSegments, sizes: *mut u64);
    /// positions[S + 1], time_keys[S], pcs[S + 1], first_call[S + 1]; a NULL array is skipped
    pub fn pw_execution_segments_read_bounds(e: *const PwExecutionSegments, positions: *mut u64, time_keys: *mut u64, pcs: *mut u32, first_call: *mut u64);
    /// rows[S x (n_airs + n_apcs)]: the class counts of every segment
    pub fn pw_execution_segments_read_heights(e: *const PwExecutionSegments, rows: *mut u64);
    /// the row list of (segment, air) on the device, what `PwGatherJob::idx` takes: 1, 0 = no rows, -1 = out of range
    pub fn pw_execution_segments_rows(e: *const PwExecutionSegments, segment: u32, air: u32, d_idx: *mut *const u32, rows: *mut u64,
                                      log_height: *mut u32) -> c_int;
    /// a host copy of all row lists (one allocation of sizes[5] bytes) and the device address of its first word
    pub fn pw_execution_segments_read_lists(e: *const PwExecutionSegments, words: *mut u32, d_base: *mut *const u32) -> c_int;
    /// out[6]: segments, classes, cell-bound probes, cuts snapped to a call's start, peak scratch, scratch held
    pub fn pw_execution_segments_last_stats(out: *mut u64);
    /// the same cut with the system AIRs' heights metered: distinct memory blocks, Merkle nodes and the Poseidon2
    /// bound as further limits; `status` 15 = a memory-bus tuple that has no key (`info` = the packed witness)
    pub fn pw_execution_segments_from_traces_metered(airs: *const PwSegmentAir, segment_of_air: *const u32, n_airs: usize, bridge_bus: u32, final_pc: u32,
                                                     cycle_counts: *const u32, apc_widths: *const u32, n_apcs: usize, call_apc_ids: *const u32,
                                                     call_from: *const u64, call_to: *const u64, n_calls: usize, limits: *const PwSegmentLimits,
                                                     meter: *const PwSystemMeter, scratch_bytes: usize, out: *mut *mut PwExecutionSegments,
                                                     status: *mut u32, info: *mut u64) -> c_int;
    /// rows[S x 3] = B, M, 2 M of every segment (zeros for a handle of the unmetered cut)
    pub fn pw_execution_segments_read_system_heights(e: *const PwExecutionSegments, rows: *mut u64);
    /// out[6]: accesses walked, tiles, the node table's most slots, nodes inserted past the cuts, host synchronisations, tables cleared
    pub fn pw_execution_segments_last_meter_stats(out: *mut u64);
    /// a test knob of the calling thread: the positions of one tile of the meter (0 = the default)
    pub fn pw_execution_segments_set_meter_tile(n: u64);
    /// the sparse memory Merkle tree: NULL unless 1 <= height <= 40
    pub fn pw_memory_tree_create(height: u32) -> *mut PwMemoryTree;
    pub fn pw_memory_tree_destroy(tree: *mut PwMemoryTree);
    /// the root as 8 canonical words on the host
    pub fn pw_memory_tree_root(tree: *const PwMemoryTree, out: *mut u32) -> c_int;
    pub fn pw_memory_tree_stats(tree: *const PwMemoryTree, out: *mut PwMemoryTreeStats) -> c_int;
    /// `status` 0 = the tree holds `d_fin`; 1 = `cap_log_height` too small; 3 = `d_init` is not what the tree holds (`info` = the key);
    /// 4 / 5 = malformed keys / payloads (`info` = the index). `d_init` NULL: load mode, no records.
    pub fn pw_memory_tree_update(tree: *mut PwMemoryTree, d_keys: *const u64, d_init: *const u32, d_fin: *const u32, n: usize,
                                 d_records: *mut u32, d_node_ids: *mut u64, cap_log_height: u32, log_height: *mut u32, n_rows: *mut u64,
                                 status: *mut u32, info: *mut u64) -> c_int;
    /// `PW_MEMORY_TREE_REBUILD` (the default) or `PW_MEMORY_TREE_INCREMENTAL`: how an update makes the levels above level 0; the
    /// results are the same bytes. No GPU call; -1 for an unknown mode or changed round constants.
    pub fn pw_memory_tree_set_mode(tree: *mut PwMemoryTree, mode: u32) -> c_int;
    pub fn pw_memory_tree_get_mode(tree: *const PwMemoryTree, mode: *mut u32) -> c_int;
    /// keys and payloads of the rows of a memory boundary trace
    pub fn pw_memory_tree_boundary_leaves(d_boundary_trace: *const u32, log_height: u32, n_locations: u64, d_keys: *mut u64,
                                          d_init: *mut u32, d_fin: *mut u32) -> c_int;
    /// the multi-opening of `n` leaves, read-only: payloads (`n` x 8, zero where a key is not stored) and the minimal sibling digests, by
    /// level and index; `status` 0 = written, 1 = `cap_siblings` too small (`n_siblings` is set), 4 = malformed keys (`info` = the index)
    pub fn pw_memory_tree_open(tree: *const PwMemoryTree, d_keys: *const u64, n: usize, d_payloads: *mut u32, d_siblings: *mut u32,
                               cap_siblings: u64, n_siblings: *mut u64, status: *mut u32, info: *mut u64) -> c_int;
    /// host only: 0 = the opening (canonical words) hashes to `root`, 19 = malformed (`where_`: the first bad key or word), 20 = another root
    pub fn pw_memory_opening_verify(height: u32, root: *const u32, keys: *const u64, payloads: *const u32, n: usize, siblings: *const u32,
                                    m: usize, where_: *mut usize) -> c_int;
    /// the memory Merkle AIR's trace (55 columns, one row per touched node, the root first) from the records and node ids of one
    /// `pw_memory_tree_update`; `status` 0 = written, 1 = `cap_log_height` too small, 2 = no rows, 3 = the ids are not a records set
    pub fn pw_memory_merkle_trace(d_records: *const u32, records_log_height: u32, d_node_ids: *const u64, n_rows: u64, height: u32,
                                  d_trace_out: *mut u32, cap_log_height: u32, log_height: *mut u32, n_nodes: *mut u64,
                                  status: *mut u32) -> c_int;
    pub fn pw_verify(cfg: *const PwStarkConfig, width: u32, log_height: u32, cons_bytecode: *const u32, bytecode_len: usize,
                     cons_spans: *const u32, n_constraints: usize, proof_words: *const u32, n_words: usize) -> c_int;
    pub fn pw_verify_logup(cfg: *const PwStarkConfig, width: u32, log_height: u32, cons_bytecode: *const u32,
                           bytecode_len: usize, cons_spans: *const u32, n_constraints: usize, interactions: *const u32,
                           n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                           inter_bytecode: *const u32, inter_bytecode_len: usize, expected_bus_seed: *const u32,
                           proof_words: *const u32, n_words: usize, cumulative_sum: *mut u32, trace_root: *mut u32) -> c_int;
    pub fn pw_logup_group_starts(interactions: *const u32, n_interactions: usize, inter_spans: *const u32,
                                 n_inter_spans: usize, inter_bytecode: *const u32, inter_bytecode_len: usize,
                                 out: *mut u32, cap: usize) -> usize;
    pub fn pw_prove_segment(airs: *const PwSegmentAir, n_airs: usize, logup: c_int, proof_words: *mut *const u32,
                            n_words: *mut usize) -> c_int;
    /// Same proof, same words; AIRs flagged `PW_AIR_HAND_OVER` that are proven STREAMED keep their coefficient arrays in the caller's buffer.
    pub fn pw_prove_segment_consuming(airs: *const PwSegmentAir, n_airs: usize, logup: c_int, proof_words: *mut *const u32,
                                      n_words: *mut usize) -> c_int;
    /// the specialised kernels of n provers in one concurrent compile batch, whatever the heights; returns how many are specialised
    pub fn pw_provers_specialise(provers: *const *mut PwProver, n: usize) -> usize;
    /// per AIR of the calling thread's last segment proof: log2(#sub-cosets) | 0x100 if the trace was overwritten (out may be null)
    pub fn pw_segment_last_modes(out: *mut u32, cap: usize) -> usize;
    /// bytes of the last segment proof's memory plan: all AIRs resident | as chosen | available to the policy
    pub fn pw_segment_last_plan(resident_bytes: *mut usize, planned_bytes: *mut usize, available_bytes: *mut usize);
    /// device bytes the calling thread's segment context holds (with its provers' bytes: at most the planned bytes)
    pub fn pw_segment_context_bytes() -> usize;
    /// bytes ONE proof call may plan for, over what its provers and the thread's segment context hold (0 = what the device has
    /// free); concurrent calls each get the whole budget
    pub fn pw_set_device_budget(bytes: usize);
    pub fn pw_get_device_budget() -> usize;
    pub fn pw_verify_segment(cfg: *const PwStarkConfig, airs: *const PwAirDescription, n_airs: usize, logup: c_int,
                             proof_words: *const u32, n_words: usize, check_balance: c_int, total_sum4: *mut u32) -> c_int;
    pub fn pw_verify_segment_preprocessed(cfg: *const PwStarkConfig, airs: *const PwAirDescription, pre: *const PwAirPreprocessed,
                                          n_airs: usize, logup: c_int, proof_words: *const u32, n_words: usize, check_balance: c_int,
                                          total_sum4: *mut u32) -> c_int;
    pub fn pw_verify_segment_transition(cfg: *const PwStarkConfig, airs: *const PwAirDescription, pre: *const PwAirPreprocessed,
                                        n_airs: usize, logup: c_int, proof_words: *const u32, n_words: usize, check_balance: c_int,
                                        total_sum4: *mut u32) -> c_int;
    /// 17 = the proof's public values differ from `expected`; pub null or every n 0: `pw_verify_segment_transition`
    pub fn pw_verify_segment_public(cfg: *const PwStarkConfig, airs: *const PwAirDescription, pre: *const PwAirPreprocessed,
                                    pub_: *const PwAirPublic, n_airs: usize, logup: c_int, proof_words: *const u32, n_words: usize,
                                    check_balance: c_int, total_sum4: *mut u32) -> c_int;
    pub fn pw_segment_proof_public_values(airs: *const PwAirDescription, pub_: *const PwAirPublic, n_airs: usize, proof_words: *const u32,
                                          n_words: usize, air: usize, out: *mut u32, cap: usize) -> usize;
    /// 0; a segment's verifier code with `where_` = its index; 18 = a link fails, `where_` = s * n_links + link
    pub fn pw_verify_segment_chain(cfg: *const PwStarkConfig, segments: *const PwChainSegment, n_segments: usize, links: *const PwChainLink,
                                   n_links: usize, where_: *mut usize) -> c_int;
    pub fn pw_prove_airs(airs: *const PwSegmentAir, n_airs: usize, shared_bus_seed: c_int, n_workers: c_uint,
                         proofs: *mut *const u32, n_words: *mut usize, bus_seed8: *mut u32) -> c_int;
    pub fn pw_verify_airs(cfg: *const PwStarkConfig, airs: *const PwAirDescription, n_airs: usize,
                          proofs: *const *const u32, n_words: *const usize, shared_bus_seed: c_int,
                          check_balance: c_int, total_sum4: *mut u32) -> c_int;
    pub fn pw_commitment_digest(roots8: *const u32, n: usize, digest8: *mut u32);
    pub fn pw_prover_reserve(p: *mut PwProver, log_height: u32) -> c_int;
    /// 0 = a proof of this height keeps the LDE resident, b >= 1 = streamed over 2^b sub-cosets, -1 = does not fit.
    pub fn pw_prover_stream_log_blocks(p: *const PwProver, log_height: u32) -> c_int;
    pub fn pw_prover_max_constraint_degree(p: *const PwProver) -> c_int;
    pub fn pw_prover_width(p: *const PwProver) -> u32;
    pub fn pw_prover_device_bytes(p: *const PwProver) -> usize;
    pub fn pw_lde_batch(d_trace: *const u32, width: u32, log_height: u32, d_coeffs: *mut u32, d_lde: *mut u32) -> c_int;
    pub fn pw_lde_fused(d_trace: *const u32, width: u32, log_height: u32, d_tmp: *mut u32, d_lde: *mut u32) -> c_int;
    pub fn pw_lde_subcoset(d_coeffs: *const u32, width: u32, log_height: u32, log_blocks: u32, r: u32, d_scale: *mut u32, d_out: *mut u32) -> c_int;
    pub fn pw_merkle_commit(d_matrix: *const u32, height: usize, width: u32, d_digests: *mut u32) -> c_int;
    pub fn pw_merkle_leaf_hash(d_matrix: *const u32, height: usize, width: u32, col_stride: usize, d_digests: *mut u32, digest_stride: usize, digest_offset: usize) -> c_int;
    pub fn pw_merkle_leaf_absorb(d_matrix: *const u32, col_stride: usize, d_cols: *const *const u32, n_cols: u32, pos0: u32, height: usize, row_stride: usize, row_offset: usize, d_state: *mut u32, d_digests: *mut u32, first: c_int, last: c_int) -> c_int;
    pub fn pw_merkle_commit_mixed(d_cols: *const *const u32, n_cols_by_log: *const u32, external_by_log: *const u32, l: u32, d_digests: *mut u32, d_inject: *mut u32) -> c_int;
    pub fn pw_merkle_commit_ext_pairs(d_values: *const u32, half: usize, d_digests: *mut u32) -> c_int;
    // single stages of the opening, DEEP, FRI, scan and layout kernels (tests and measurement only; scalars: host, 4 canonical words)
    pub fn pw_stage_opening_weights(zeta: *const u32, log_h: u32, on_coefficients: c_int, d_w: *mut u32) -> c_int;
    pub fn pw_stage_ext_dot(d_cols: *const u32, stride: usize, n_cols: u32, len: usize, d_w: *const u32, d_w2: *const u32, d_out: *mut u32, d_out2: *mut u32) -> c_int;
    pub fn pw_stage_ext_powers(base: *const u32, n: u32, reversed: c_int, centred: c_int, d_out: *mut u32) -> c_int;
    pub fn pw_stage_deep(d_a: *const u32, wa: u32, d_b: *const u32, wb: u32, log_n: u32, d_gpow: *const u32, sum: *const u32, zeta: *const u32, d_v: *mut u32) -> c_int;
    pub fn pw_stage_deep_logup(d_lde: *const u32, w: u32, d_plde: *const u32, wp: u32, d_qlde: *const u32, log_n: u32, d_gpow: *const u32, g_k: *const u32,
                               sum1: *const u32, sum2: *const u32, zeta: *const u32, gzeta: *const u32, d_v: *mut u32) -> c_int;
    pub fn pw_stage_ext_lincomb(d_a: *const u32, wa: u32, d_b: *const u32, wb: u32, len: usize, d_gpow: *const u32, second: u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_deep_from_combo(d_glde: *const u32, d_qlde: *const u32, log_n: u32, d_gq: *const u32, sum1: *const u32, sum2: *const u32,
                                    zeta: *const u32, gzeta: *const u32, two: c_int, d_v: *mut u32) -> c_int;
    pub fn pw_stage_fri_fold(d_v: *const u32, log_size: u32, shift: u32, beta: *const u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_logup_scan(d_rowsum: *const u32, h: usize, d_phi_cols: *mut u32) -> c_int;
    pub fn pw_stage_quotient_split(d_cbr: *const u32, log_h: u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_row_layout(d_m: *mut u32, log_n: u32, w1: u32, d_next_cols: *const u32, n_next: u32, step: u32, selectors: c_int, trace_domain: c_int) -> c_int;
    pub fn pw_stage_part_scatter(d_part: *const u32, n_chunks: u32, m: usize, b: u32, r: u32, n: usize, d_out: *mut u32) -> c_int;
    pub fn pw_stage_ext_axpy(d_y: *mut u32, a: *const u32, d_x: *const u32, n: usize) -> c_int;
    pub fn pw_stage_logup_perm(p: *mut PwProver, d_values: *const u32, log_h: u32, alpha: *const u32, d_blpow: *const u32, d_perm: *mut u32,
                               d_rowsum: *mut u32) -> c_int;
    pub fn pw_stage_quotient(p: *mut PwProver, d_lde: *const u32, d_plde: *const u32, log_n: u32, d_apow: *const u32, alpha: *const u32,
                             d_blpow: *const u32, s: *const u32, d_q: *mut u32, n_chunks_out: *mut u32) -> c_int;
    pub fn pw_stage_quotient_sums(p: *mut PwProver, d_t: *const u32, d_pm: *const u32, rows: usize, log_n: u32, d_apow: *const u32,
                                  alpha: *const u32, d_blpow: *const u32, unit: c_int, d_part: *mut u32, n_parts_out: *mut u32) -> c_int;
    pub fn pw_stage_logup_tail(d_part: *const u32, n_chunks: u32, d_plde_phi: *const u32, d_plde_sumq: *const u32, log_n: u32,
                               d_apow_tail: *const u32, s: *const u32, d_q: *mut u32) -> c_int;
    pub fn pw_stage_rowsum_combine(d_part: *const u32, n_chunks: u32, h: usize, d_rowsum: *mut u32, d_cols4: *mut u32) -> c_int;
    pub fn pw_prover_quotient_units(p: *const PwProver) -> u32;
    pub fn pw_prover_quotient_unit_groups(p: *const PwProver, unit: u32, g0: *mut u32, g1: *mut u32) -> c_int;
    pub fn pw_stage_pow_grind(state16: *const u32, pending: *const u32, in_len: u32, bits: u32, witness_out: *mut u32) -> c_int;
    pub fn pw_stage_gather_rows(d_m: *const u32, height: usize, width: u32, d_idx: *const u32, n_idx: u32, canonical: c_int, d_out: *mut u32) -> c_int;
    pub fn pw_stage_canonicalize(d_words: *mut u32, n: usize) -> c_int;
    pub fn pw_stage_gather_rows_multi(jobs: *const PwStageGatherJob, n_jobs: u32, d_idx: *const u32, n_idx: u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_gather_records(d_arena: *const u32, offsets: *const u64, words_per_record: u32, n: u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_gather_words(d_ptrs: *const *const u32, n: u32, d_out: *mut u32) -> c_int;
    pub fn pw_stage_ext_to_cols(d_in: *const u32, len: usize, d_cols4: *mut u32) -> c_int;
    pub fn pw_stage_query_rows(d_coeffs: *const u32, cols: u32, log_h: u32, log_blocks: u32, idx: *const u32, n_idx: u32, d_work: *mut u32,
                               work_words: usize, select_words: usize, d_scale: *mut u32, d_rows: *mut u32, forms: *mut u8) -> c_int;
    pub fn pw_prover_specialise(p: *mut PwProver) -> c_int;
    pub fn pw_prover_specialised(p: *const PwProver, n_kernels: *mut usize, code_bytes: *mut usize, n_chunks: *mut usize) -> c_int;
    pub fn pw_prove_segments_multi(devices: *const c_int, n_workers: usize, segment_cells: *const u64, n_segments: usize,
                                   prove: PwSegmentProveFn, user: *mut c_void, commitments: *mut u32, worker_of_segment: *mut u32) -> c_int;
    pub fn pw_multi_last_merge() -> c_int;
    pub fn pw_assign_units(cells: *const u64, n_units: usize, n_workers: usize, worker_of_unit: *mut u32) -> usize;
    pub fn pw_jit_generated_source(width: u32, cons_bytecode: *const u32, bytecode_len: usize, cons_spans: *const u32, n_constraints: usize,
                                   interactions: *const u32, n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                   inter_bytecode: *const u32, inter_bytecode_len: usize, which: c_int, chunk_cost: u32, chunks_per_unit: u32,
                                   unit: usize, buf: *mut c_char, cap: usize, kernel_name: *mut c_char, name_cap: usize, first_chunk: *mut u32,
                                   n_chunks: *mut u32, total_chunks: *mut u32) -> usize;
    pub fn pw_jit_cache_stats(units_compiled: *mut u64, units_from_disk: *mut u64);
    pub fn pw_jit_compile_check(width: u32, cons_bytecode: *const u32, bytecode_len: usize, cons_spans: *const u32, n_constraints: usize,
                                interactions: *const u32, n_interactions: usize, inter_spans: *const u32, n_inter_spans: usize,
                                inter_bytecode: *const u32, inter_bytecode_len: usize, n_kernels: *mut usize, code_bytes: *mut usize,
                                n_chunks: *mut usize, err: *mut c_char, err_cap: usize) -> c_int;
    pub fn pw_poseidon2_permute_host(state16: *mut u32);
    pub fn pw_set_poseidon2_constants(ext_rc: *const u32, int_rc: *const u32) -> c_int;
    pub fn pw_get_poseidon2_constants(ext_rc: *mut u32, int_rc: *mut u32, diag: *mut u32);
}

// --------------------------------------------------------------------------------- HIP runtime (libamdhip64), minimal
extern "C" {
    pub fn hipMalloc(ptr: *mut *mut c_void, bytes: usize) -> c_int;
    pub fn hipFree(ptr: *mut c_void) -> c_int;
    pub fn hipMemcpy(dst: *mut c_void, src: *const c_void, bytes: usize, kind: c_int) -> c_int;
    pub fn hipMemset(dst: *mut c_void, value: c_int, bytes: usize) -> c_int;
    pub fn hipDeviceSynchronize() -> c_int;
    pub fn hipSetDevice(device: c_int) -> c_int;
}
pub const HIP_MEMCPY_HOST_TO_DEVICE: c_int = 1;
pub const HIP_MEMCPY_DEVICE_TO_HOST: c_int = 2;
