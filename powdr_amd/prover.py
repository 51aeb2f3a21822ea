"""ctypes binding of the pw-stark v0 prover entry points (include/powdr_prover.h)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, stage

lib = abi.lib


class PwStarkConfig(C.Structure):
    _fields_ = [("num_queries", C.c_uint32), ("pow_bits", C.c_uint32)]


class PwStageGatherJob(C.Structure):
    """One matrix of pw_stage_gather_rows_multi (include/powdr_prover.h)."""
    _fields_ = [("d_m", C.c_void_p), ("height", C.c_uint64), ("width", C.c_uint32), ("idx_off", C.c_uint32), ("out_off", C.c_uint64)]


PROVER_SYMBOLS = ["pw_prover_check_constraints", "pw_verify", "pw_prover_create", "pw_prover_create_logup", "pw_verify_logup", "pw_prover_trace_root", "pw_prover_set_bus_seed", "pw_prover_logup_path", "pw_prove_airs", "pw_verify_airs", "pw_prove_segment", "pw_verify_segment", "pw_commitment_digest", "pw_logup_group_starts", "pw_prover_width", "pw_prover_reserve", "pw_prover_stream_log_blocks", "pw_prover_max_constraint_degree", "pw_prover_destroy", "pw_prover_prove", "pw_prover_prove_consuming", "pw_prover_stream_log_blocks_consuming", "pw_trace_from_coefficients", "pw_prover_device_bytes",
                  "pw_lde_batch", "pw_lde_fused", "pw_lde_subcoset", "pw_merkle_commit", "pw_poseidon2_permute_host",
                  "pw_merkle_leaf_hash", "pw_merkle_leaf_absorb", "pw_merkle_commit_mixed", "pw_merkle_commit_ext_pairs",
                  "pw_stage_opening_weights", "pw_stage_ext_dot", "pw_stage_ext_powers", "pw_stage_deep", "pw_stage_deep_logup",
                  "pw_stage_ext_lincomb", "pw_stage_deep_from_combo", "pw_stage_fri_fold", "pw_stage_logup_scan", "pw_stage_quotient_split",
                  "pw_stage_row_layout", "pw_stage_part_scatter", "pw_stage_ext_axpy",
                  "pw_stage_logup_perm", "pw_stage_quotient", "pw_stage_quotient_sums", "pw_stage_logup_tail", "pw_stage_rowsum_combine",
                  "pw_prover_quotient_units", "pw_prover_quotient_unit_groups",
                  "pw_stage_pow_grind", "pw_stage_gather_rows", "pw_stage_canonicalize", "pw_stage_gather_rows_multi", "pw_stage_gather_records",
                  "pw_stage_gather_words", "pw_stage_ext_to_cols", "pw_stage_query_rows",
                  "pw_set_poseidon2_constants", "pw_get_poseidon2_constants", "pw_prover_specialise", "pw_prover_specialised", "pw_jit_compile_check", "pw_jit_cache_stats", "pw_jit_generated_source",
                  "pw_prove_segments_multi", "pw_multi_last_merge", "pw_assign_units",
                  "pw_prove_segment_consuming", "pw_segment_last_modes", "pw_segment_last_plan", "pw_set_device_budget", "pw_get_device_budget", "pw_provers_specialise",
                  "pw_segment_context_bytes", "pw_segment_stream_plan", "pw_segment_last_plan_tables",
                  "pw_prover_create_preprocessed", "pw_prover_preprocessed_root", "pw_prover_preprocessed_width", "pw_verify_segment_preprocessed",
                  "pw_prover_create_transition", "pw_prover_row_flags", "pw_verify_segment_transition",
                  "pw_prover_create_public", "pw_prover_n_public", "pw_prover_set_public_values", "pw_verify_segment_public",
                  "pw_segment_proof_public_values", "pw_verify_segment_chain", "pw_public_programs_check",
                  "pw_check_segment_buses", "pw_bus_check_scratch_bytes", "pw_bus_check_peak_bytes", "pw_bus_check_last_stats",
                  "pw_poseidon2_compress_trace",
                  "pw_memory_tree_create", "pw_memory_tree_destroy", "pw_memory_tree_root", "pw_memory_tree_stats", "pw_memory_tree_update",
                  "pw_memory_tree_boundary_leaves", "pw_memory_tree_set_mode", "pw_memory_tree_get_mode",
                  "pw_memory_merkle_trace", "pw_memory_tree_open", "pw_memory_opening_verify"]

lib.pw_prover_create.restype = C.c_void_p
lib.pw_prover_create.argtypes = [C.POINTER(PwStarkConfig), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
lib.pw_prover_create_logup.restype = C.c_void_p
lib.pw_prover_create_logup.argtypes = [C.POINTER(PwStarkConfig), C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
lib.pw_prover_destroy.argtypes = [C.c_void_p]
lib.pw_prover_create_preprocessed.restype = C.c_void_p
lib.pw_prover_create_preprocessed.argtypes = [C.POINTER(PwStarkConfig), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
lib.pw_prover_preprocessed_root.restype = C.c_int
lib.pw_prover_preprocessed_root.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_prover_preprocessed_width.restype = C.c_uint32
lib.pw_prover_preprocessed_width.argtypes = [C.c_void_p]
lib.pw_prover_create_transition.restype = C.c_void_p
lib.pw_prover_create_transition.argtypes = lib.pw_prover_create_preprocessed.argtypes
lib.pw_prover_row_flags.restype = C.c_uint32
lib.pw_prover_row_flags.argtypes = [C.c_void_p]
lib.pw_prover_create_public.restype = C.c_void_p
lib.pw_prover_create_public.argtypes = lib.pw_prover_create_preprocessed.argtypes[:5] + [C.c_uint32] + lib.pw_prover_create_preprocessed.argtypes[5:]
lib.pw_prover_n_public.restype = C.c_uint32
lib.pw_prover_n_public.argtypes = [C.c_void_p]
lib.pw_prover_set_public_values.restype = C.c_int
lib.pw_prover_set_public_values.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
lib.pw_prover_prove.restype = C.c_int
lib.pw_prover_prove.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
lib.pw_prover_check_constraints.restype = C.c_int
lib.pw_prover_check_constraints.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint32)]
lib.pw_prover_device_bytes.restype = C.c_size_t
lib.pw_prover_device_bytes.argtypes = [C.c_void_p]
lib.pw_lde_batch.restype = C.c_int
lib.pw_lde_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.pw_lde_fused.restype = C.c_int
lib.pw_lde_fused.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.pw_prover_prove_consuming.restype = C.c_int
lib.pw_prover_prove_consuming.argtypes = lib.pw_prover_prove.argtypes
lib.pw_prover_stream_log_blocks_consuming.restype = C.c_int
lib.pw_prover_stream_log_blocks_consuming.argtypes = [C.c_void_p, C.c_uint32]
lib.pw_trace_from_coefficients.restype = C.c_int
lib.pw_trace_from_coefficients.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.pw_lde_subcoset.restype = C.c_int
lib.pw_lde_subcoset.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
lib.pw_segment_last_modes.restype = C.c_size_t
lib.pw_segment_last_modes.argtypes = [C.c_void_p, C.c_size_t]
lib.pw_segment_context_bytes.restype = C.c_size_t
lib.pw_segment_context_bytes.argtypes = []
lib.pw_segment_stream_plan.restype = C.c_size_t
lib.pw_segment_stream_plan.argtypes = [C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p]
lib.pw_segment_last_plan_tables.restype = C.c_size_t
lib.pw_segment_last_plan_tables.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
lib.pw_set_device_budget.restype = None
lib.pw_set_device_budget.argtypes = [C.c_size_t]
lib.pw_get_device_budget.restype = C.c_size_t
lib.pw_merkle_commit.restype = C.c_int
lib.pw_merkle_commit.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p]
lib.pw_merkle_leaf_hash.restype = C.c_int
lib.pw_merkle_leaf_hash.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t]
lib.pw_merkle_leaf_absorb.restype = C.c_int
lib.pw_merkle_leaf_absorb.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_int, C.c_int]
lib.pw_merkle_commit_mixed.restype = C.c_int
lib.pw_merkle_commit_mixed.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
lib.pw_merkle_commit_ext_pairs.restype = C.c_int
lib.pw_merkle_commit_ext_pairs.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
lib.pw_poseidon2_permute_host.argtypes = [C.c_void_p]
# the stage entry points of the opening, DEEP, FRI, scan and layout kernels (include/powdr_prover.h): device pointers and host
# pointers to 4 canonical words alike travel as c_void_p
_STAGE_ARGTYPES = {
    "pw_stage_opening_weights": [C.c_void_p, C.c_uint32, C.c_int, C.c_void_p],
    "pw_stage_ext_dot": [C.c_void_p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "pw_stage_ext_powers": [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p],
    "pw_stage_deep": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "pw_stage_deep_logup": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                            C.c_void_p, C.c_void_p, C.c_void_p],
    "pw_stage_ext_lincomb": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p],
    "pw_stage_deep_from_combo": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p],
    "pw_stage_fri_fold": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p],
    "pw_stage_logup_scan": [C.c_void_p, C.c_size_t, C.c_void_p],
    "pw_stage_quotient_split": [C.c_void_p, C.c_uint32, C.c_void_p],
    "pw_stage_row_layout": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int],
    "pw_stage_part_scatter": [C.c_void_p, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p],
    "pw_stage_ext_axpy": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t],
    # the LogUp permutation and quotient stages of one prover (the first argument: Prover._h)
    "pw_stage_logup_perm": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "pw_stage_quotient": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                          C.POINTER(C.c_uint32)],
    "pw_stage_quotient_sums": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                               C.POINTER(C.c_uint32)],
    "pw_stage_logup_tail": [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p],
    "pw_stage_rowsum_combine": [C.c_void_p, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p],
    # the query phase: grinding (host words in, the witness out), the gathers, a streamed AIR's rows (host indices, a byte per sub-coset out)
    "pw_stage_pow_grind": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32)],
    "pw_stage_gather_rows": [C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p],
    "pw_stage_canonicalize": [C.c_void_p, C.c_size_t],
    "pw_stage_gather_rows_multi": [C.POINTER(PwStageGatherJob), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p],
    "pw_stage_gather_records": [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p],
    "pw_stage_gather_words": [C.c_void_p, C.c_uint32, C.c_void_p],
    "pw_stage_ext_to_cols": [C.c_void_p, C.c_size_t, C.c_void_p],
    "pw_stage_query_rows": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p,
                            C.c_void_p, C.c_void_p],
}
for _name, _argtypes in _STAGE_ARGTYPES.items():
    getattr(lib, _name).restype = C.c_int
    getattr(lib, _name).argtypes = _argtypes
lib.pw_prover_quotient_units.restype = C.c_uint32
lib.pw_prover_quotient_units.argtypes = [C.c_void_p]
lib.pw_prover_quotient_unit_groups.restype = C.c_int
lib.pw_prover_quotient_unit_groups.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _interaction_tables(interactions):
    """interactions = (inter[n x 3] = {bus, n_args, first span}, spans[m x 2], bytecode) or None -> the six (pointer, length) arguments
    the C entry points take for them, and the arrays those pointers point into."""
    if interactions is None:
        return (None, 0, None, 0, None, 0), []
    it = np.ascontiguousarray(interactions[0], dtype=np.uint32).reshape(-1, 3)
    isp = np.ascontiguousarray(interactions[1], dtype=np.uint32).reshape(-1, 2)
    ibc = np.ascontiguousarray(interactions[2], dtype=np.uint32)
    return (_vp(it), len(it), _vp(isp), len(isp), _vp(ibc), len(ibc)), [it, isp, ibc]


lib.pw_verify.restype = C.c_int
lib.pw_verify.argtypes = [C.POINTER(PwStarkConfig), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                          C.c_void_p, C.c_size_t]


def verify(proof, width: int, log_height: int, cons_bytecode, cons_spans, num_queries: int = 100, pow_bits: int = 0) -> int:
    """Host-side verification (no GPU). 0 = valid, otherwise the code of the first failed check."""
    pr = np.ascontiguousarray(proof, dtype=np.uint32)
    bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
    sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
    cfg = PwStarkConfig(num_queries, pow_bits)
    return int(lib.pw_verify(C.byref(cfg), width, log_height, bc.ctypes.data_as(C.c_void_p), len(bc),
                             sp.ctypes.data_as(C.c_void_p), len(sp), pr.ctypes.data_as(C.c_void_p), len(pr)))


lib.pw_verify_logup.restype = C.c_int
lib.pw_verify_logup.argtypes = [C.POINTER(PwStarkConfig), C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t,
                                C.c_void_p, C.c_void_p]
lib.pw_prover_trace_root.restype = C.c_int
lib.pw_prover_trace_root.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
lib.pw_prover_logup_path.restype = C.c_int
lib.pw_prover_logup_path.argtypes = [C.c_void_p]
lib.pw_prover_set_bus_seed.restype = C.c_int
lib.pw_prover_set_bus_seed.argtypes = [C.c_void_p, C.c_void_p]


def verify_logup(proof, width: int, log_height: int, cons_bytecode, cons_spans, interactions, num_queries: int = 100,
                 pow_bits: int = 0, bus_seed=None, with_root: bool = False):
    """Host-side verification of a LogUp proof: (code, cumulative bus sum S as 4 canonical words or None)
    [, trace root]. bus_seed: the 8 words the proof must have drawn its bus challenges from (None: its own
    trace root)."""
    pr = np.ascontiguousarray(proof, dtype=np.uint32)
    bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
    sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
    tables, _ = _interaction_tables(interactions)
    cfg = PwStarkConfig(num_queries, pow_bits)
    s, root = np.zeros(4, np.uint32), np.zeros(8, np.uint32)
    p = _vp
    seed = None if bus_seed is None else np.ascontiguousarray(bus_seed, dtype=np.uint32)
    rc = int(lib.pw_verify_logup(C.byref(cfg), width, log_height, p(bc), len(bc), p(sp), len(sp), *tables,
                                 None if seed is None else p(seed), p(pr), len(pr), p(s), p(root)))
    if with_root:
        return rc, (s if rc == 0 else None), (root if rc == 0 else None)
    return rc, (s if rc == 0 else None)


PwSegmentAir = stage.PwSegmentAir


PW_AIR_HAND_OVER = 1


class PwAirDescription(C.Structure):
    _fields_ = [("width", C.c_uint32), ("log_height", C.c_uint32), ("logup", C.c_uint32),
                ("cons_bytecode", C.c_void_p), ("bytecode_len", C.c_size_t), ("cons_spans", C.c_void_p), ("n_constraints", C.c_size_t),
                ("interactions", C.c_void_p), ("n_interactions", C.c_size_t), ("inter_spans", C.c_void_p), ("n_inter_spans", C.c_size_t),
                ("inter_bytecode", C.c_void_p), ("inter_bytecode_len", C.c_size_t)]


lib.pw_prove_airs.restype = C.c_int
lib.pw_prove_airs.argtypes = [C.POINTER(PwSegmentAir), C.c_size_t, C.c_int, C.c_uint, C.POINTER(C.POINTER(C.c_uint32)),
                                 C.POINTER(C.c_size_t), C.c_void_p]
lib.pw_prove_segment.restype = C.c_int
lib.pw_prove_segment.argtypes = [C.POINTER(PwSegmentAir), C.c_size_t, C.c_int, C.POINTER(C.POINTER(C.c_uint32)), C.POINTER(C.c_size_t)]
lib.pw_prove_segment_consuming.restype = C.c_int
lib.pw_prove_segment_consuming.argtypes = lib.pw_prove_segment.argtypes
lib.pw_verify_segment.restype = C.c_int
lib.pw_verify_segment.argtypes = [C.POINTER(PwStarkConfig), C.POINTER(PwAirDescription), C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]


class PwAirPreprocessed(C.Structure):
    _fields_ = [("width", C.c_uint32), ("root8", C.c_uint32 * 8)]


lib.pw_verify_segment_preprocessed.restype = C.c_int
lib.pw_verify_segment_preprocessed.argtypes = [C.POINTER(PwStarkConfig), C.POINTER(PwAirDescription), C.POINTER(PwAirPreprocessed), C.c_size_t, C.c_int,
                                               C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
lib.pw_verify_segment_transition.restype = C.c_int
lib.pw_verify_segment_transition.argtypes = lib.pw_verify_segment_preprocessed.argtypes


class PwAirPublic(C.Structure):
    _fields_ = [("n", C.c_uint32), ("expected", C.c_void_p)]


class PwChainSegment(C.Structure):
    _fields_ = [("airs", C.POINTER(PwAirDescription)), ("pre", C.POINTER(PwAirPreprocessed)), ("pub", C.POINTER(PwAirPublic)), ("n_airs", C.c_size_t),
                ("logup", C.c_int), ("proof", C.c_void_p), ("n_words", C.c_size_t), ("check_balance", C.c_int)]


class PwChainLink(C.Structure):
    _fields_ = [("air_from", C.c_uint32), ("index_from", C.c_uint32), ("air_to", C.c_uint32), ("index_to", C.c_uint32)]


lib.pw_verify_segment_public.restype = C.c_int
lib.pw_verify_segment_public.argtypes = [C.POINTER(PwStarkConfig), C.POINTER(PwAirDescription), C.POINTER(PwAirPreprocessed), C.POINTER(PwAirPublic),
                                         C.c_size_t, C.c_int, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
lib.pw_segment_proof_public_values.restype = C.c_size_t
lib.pw_segment_proof_public_values.argtypes = [C.POINTER(PwAirDescription), C.POINTER(PwAirPublic), C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t,
                                               C.c_void_p, C.c_size_t]
lib.pw_verify_segment_chain.restype = C.c_int
lib.pw_verify_segment_chain.argtypes = [C.POINTER(PwStarkConfig), C.POINTER(PwChainSegment), C.c_size_t, C.POINTER(PwChainLink), C.c_size_t,
                                        C.POINTER(C.c_size_t)]
lib.pw_public_programs_check.restype = C.c_int
lib.pw_public_programs_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                         C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint32), C.c_void_p,
                                         C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
lib.pw_verify_airs.restype = C.c_int
lib.pw_verify_airs.argtypes = [C.POINTER(PwStarkConfig), C.POINTER(PwAirDescription), C.c_size_t, C.POINTER(C.c_void_p),
                                  C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_void_p]
lib.pw_commitment_digest.restype = None
lib.pw_commitment_digest.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]


lib.pw_logup_group_starts.restype = C.c_size_t
lib.pw_logup_group_starts.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]


class RowOperands:
    """The operand layout of constraint programs with next-row reads and row selectors (pw_prover_create_transition):
    W1 = width + pre_width; c < W1 the current row, next(c) = W1 + c the next row, then is_first_row, is_last_row, is_transition."""

    def __init__(self, width: int, pre_width: int = 0):
        self.width, self.pre_width = int(width), int(pre_width)
        self.w1 = self.width + self.pre_width
        self.is_first_row, self.is_last_row, self.is_transition = 2 * self.w1, 2 * self.w1 + 1, 2 * self.w1 + 2
        self.bound = 2 * self.w1 + 3  # constraint operands below this (+ n_public: public(k)); interaction operands below w1

    def public(self, k: int) -> int:
        """public value k of the AIR (Prover(..., n_public=)): a constraint operand of degree 0"""
        if not 0 <= k < 256:
            raise ValueError(f"public value {k}: an AIR has at most 256")
        return self.bound + k

    def next(self, c: int) -> int:
        if not 0 <= c < self.w1:
            raise ValueError(f"column {c}: the current row has {self.w1} columns")
        return self.w1 + c


def row_operands(width: int, pre_width: int = 0) -> RowOperands:
    return RowOperands(width, pre_width)


def logup_group_starts(interactions) -> np.ndarray:
    """Boundaries of the LogUp groups (one committed extension column each) for an interaction table."""
    tables, _ = _interaction_tables(interactions)
    out = np.zeros(tables[1] + 2, np.uint32)
    k = lib.pw_logup_group_starts(*tables, _vp(out), len(out))
    if k == 0:
        raise ValueError("malformed interaction table")
    return out[:k].copy()


def commitment_digest(roots) -> np.ndarray:
    """Digest over an ordered list of 8-word commitments (canonical words)."""
    r = np.ascontiguousarray(roots, dtype=np.uint32).reshape(-1, 8)
    out = np.zeros(8, np.uint32)
    lib.pw_commitment_digest(r.ctypes.data_as(C.c_void_p), len(r), out.ctypes.data_as(C.c_void_p))
    return out


def prove_airs(airs, shared_bus_seed: bool = False, n_workers: int = 0, copy: bool = True):
    """airs: [(Prover, device trace pointer, log_height)] -> ([proof words per AIR], bus seed).
    INDEPENDENT proofs, one per AIR, on `n_workers` host threads / HIP streams (0 = 4) — the flow AIR-level sharding
    over ranks uses; `prove_segment` is the one-proof-per-segment form."""
    n, recs = len(airs), stage.air_records(airs)[0]
    proofs = (C.POINTER(C.c_uint32) * max(n, 1))()
    lens = (C.c_size_t * max(n, 1))()
    seed = np.zeros(8, np.uint32)
    rc = lib.pw_prove_airs(recs, n, int(shared_bus_seed), n_workers, proofs, lens, seed.ctypes.data_as(C.c_void_p))
    abi.check(rc, "pw_prove_airs")
    out = []
    for i in range(n):
        a = np.ctypeslib.as_array(proofs[i], shape=(lens[i],))
        out.append(a.copy() if copy else a)
    return out, seed


def _air_descriptions(descs):
    n = len(descs)
    keep, recs = [], (PwAirDescription * max(n, 1))()
    for i, (w, lh, bc, sp, it) in enumerate(descs):
        bc = np.ascontiguousarray(bc, dtype=np.uint32)
        sp = np.ascontiguousarray(sp, dtype=np.uint32).reshape(-1, 2)
        tables, arrays = _interaction_tables(it)
        keep += [bc, sp] + arrays  # (the record's pointer fields hold plain addresses)
        recs[i] = PwAirDescription(w, lh, 0 if it is None else 1, _vp(bc), len(bc), _vp(sp), len(sp), *tables)
    return recs, keep


def prove_segment(airs, logup: bool = False, copy: bool = True, hand_over=None) -> np.ndarray:
    """ONE proof for all AIRs of a segment (pw-stark v1, magic PWS3): airs = [(Prover, device trace pointer, log_height)],
    every Prover created with `interactions=` when logup. The counterpart of the reference's one engine call per segment.
    hand_over: None = pw_prove_segment; True / a list of bools = pw_prove_segment_consuming with those AIRs' traces handed over
    (a STREAMED AIR then leaves its coefficient arrays in the caller's buffer: segment_last_modes() says which did)."""
    n = len(airs)
    flags = [0] * n if hand_over is None else ([PW_AIR_HAND_OVER] * n if hand_over is True else [PW_AIR_HAND_OVER if f else 0 for f in hand_over])
    recs = stage.air_records(airs, flags=flags)[0]
    words = C.POINTER(C.c_uint32)()
    nw = C.c_size_t()
    if hand_over is None:
        abi.check(lib.pw_prove_segment(recs, n, int(logup), C.byref(words), C.byref(nw)), "pw_prove_segment")
    else:
        abi.check(lib.pw_prove_segment_consuming(recs, n, int(logup), C.byref(words), C.byref(nw)), "pw_prove_segment_consuming")
    a = np.ctypeslib.as_array(words, shape=(nw.value,))
    return a.copy() if copy else a


PW_BUS_MAX_ARGS = 16
PW_BUS_CHECK_TALLY_ALL = 1


class PwBusSummary(C.Structure):
    _fields_ = [("bus", C.c_uint32), ("status", C.c_uint32), ("n_active", C.c_uint64), ("n_unbalanced", C.c_uint64)]


class PwBusTuple(C.Structure):
    _fields_ = [("bus", C.c_uint32), ("n_args", C.c_uint32), ("args", C.c_uint32 * PW_BUS_MAX_ARGS), ("net_multiplicity", C.c_uint32),
                ("air", C.c_uint32), ("interaction", C.c_uint32), ("row", C.c_uint64), ("n_contributions", C.c_uint64)]


lib.pw_check_segment_buses.restype = C.c_int
lib.pw_check_segment_buses.argtypes = [C.POINTER(PwSegmentAir), C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint64, C.c_size_t, C.c_uint32,
                                       C.POINTER(PwBusSummary), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(PwBusTuple), C.c_size_t,
                                       C.POINTER(C.c_size_t)]
lib.pw_bus_check_scratch_bytes.restype = C.c_size_t
lib.pw_bus_check_scratch_bytes.argtypes = []
lib.pw_bus_check_peak_bytes.restype = C.c_size_t
lib.pw_bus_check_peak_bytes.argtypes = []
lib.pw_bus_check_last_stats.restype = None
lib.pw_bus_check_last_stats.argtypes = [C.POINTER(C.c_uint64)] * 4  # (a diagnostic of the library for tools/bench_bus_check.py, not in the header)


def check_segment_buses(airs, buses=None, seed: int = 0, table_bytes: int = 0, tally_all: bool = False, tuple_cap: int = 1024):
    """pw_check_segment_buses, the bus half of the mock prover: airs = [(Prover, device trace pointer, log_height)] as
    for prove_segment; buses = the bus ids to check (None: every id that occurs). Returns (summaries, tuples):
    summaries, by bus id: dict(bus, status, n_active, n_unbalanced) — status 0 balanced, 1 unbalanced with its tuples listed,
    2 unbalanced but the tally table (table_bytes: the most one bus's table may take; it grows to that from 2.6 MB) was too small to
    name them;
    tuples, by (bus, n_args, args): dict(bus, n_args, args (canonical, the first 16), net_multiplicity, air, interaction, row,
    n_contributions) — at most tuple_cap of them, the first in that order. A tuple is (bus, n_args, args): (a, b) is not (a, b, 0)."""
    n, recs = len(airs), stage.air_records(airs)[0]
    ids = None if buses is None else np.ascontiguousarray(sorted(set(int(b) for b in buses)), dtype=np.uint32)
    if ids is not None and len(ids) == 0:
        return [], []
    cap = len(ids) if ids is not None else 4096  # (more distinct bus ids than that: -1)
    sums = (PwBusSummary * cap)()
    tups = (PwBusTuple * max(tuple_cap, 1))()
    ns, nt = C.c_size_t(), C.c_size_t()
    rc = lib.pw_check_segment_buses(recs, n, None if ids is None else _vp(ids), 0 if ids is None else len(ids), int(seed) & (2**64 - 1),
                                    int(table_bytes), PW_BUS_CHECK_TALLY_ALL if tally_all else 0, sums, cap, C.byref(ns),
                                    tups if tuple_cap else None, tuple_cap, C.byref(nt))
    abi.check(rc, "pw_check_segment_buses")
    summaries = [dict(bus=int(s.bus), status=int(s.status), n_active=int(s.n_active), n_unbalanced=int(s.n_unbalanced)) for s in sums[:ns.value]]
    tuples = [dict(bus=int(t.bus), n_args=int(t.n_args), args=[int(x) for x in t.args[:min(t.n_args, PW_BUS_MAX_ARGS)]],
                   net_multiplicity=int(t.net_multiplicity), air=int(t.air), interaction=int(t.interaction), row=int(t.row),
                   n_contributions=int(t.n_contributions)) for t in tups[:nt.value]]
    return summaries, tuples


def bus_check_scratch_bytes() -> int:
    """device bytes this thread's bus-check scratch holds now (the tally table and the tuple lists are released after every call)"""
    return int(lib.pw_bus_check_scratch_bytes())


def bus_check_peak_bytes() -> int:
    """the most device bytes this thread's last check_segment_buses held at once (both passes)"""
    return int(lib.pw_bus_check_peak_bytes())


def bus_check_last_stats() -> dict:
    """of this thread's last check_segment_buses: slots of the largest tally table, most slots occupied in one, triples inserted,
    tables tallied into (the attempts that overflowed included)"""
    a, b, c, d = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    lib.pw_bus_check_last_stats(C.byref(a), C.byref(b), C.byref(c), C.byref(d))
    return dict(table_slots=a.value, occupied_slots=b.value, inserted=c.value, tables=d.value)


def segment_last_modes():
    """[(log2 sub-cosets, trace overwritten by its coefficients)] per AIR of this thread's last segment proof."""
    n = int(lib.pw_segment_last_modes(None, 0))
    out = (C.c_uint32 * max(n, 1))()
    lib.pw_segment_last_modes(out, n)
    return [(int(out[i]) & 0xFF, bool(int(out[i]) & 0x100)) for i in range(n)]


def segment_last_plan():
    """(bytes with every AIR resident, bytes as planned, bytes the policy had) of this thread's last segment proof."""
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    lib.pw_segment_last_plan(C.byref(a), C.byref(b), C.byref(c))
    return a.value, b.value, c.value


def segment_context_bytes() -> int:
    """pw_segment_context_bytes: device bytes this thread's segment context holds (with its provers' bytes: <= the planned bytes)."""
    return int(lib.pw_segment_context_bytes())


def segment_stream_plan(resident, streamed, b_max, own: int, avail: int):
    """The segment memory policy on given byte tables (test hook pw_segment_stream_plan): resident[n], streamed[n x 5] (column b - 1:
    2^b sub-cosets), b_max[n] (0 = may not stream) -> (log2 sub-cosets per AIR, bytes planned)."""
    n = len(resident)
    r = np.ascontiguousarray(resident, dtype=np.uint64)
    s = np.ascontiguousarray(streamed, dtype=np.uint64).reshape(n, 5)
    b = np.ascontiguousarray(b_max, dtype=np.int32)
    out = np.zeros(max(n, 1), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    need = int(lib.pw_segment_stream_plan(n, vp(r), vp(s), vp(b), int(own), int(avail), vp(out)))
    return out[:n].tolist(), need


def segment_last_plan_tables():
    """The byte tables this thread's last segment proof planned with: (resident[n], streamed[n x 5], b_max[n]); n = 0 when no policy
    ran (forced modes)."""
    n = int(lib.pw_segment_last_plan_tables(None, None, None, 0))
    r, s, b = np.zeros(max(n, 1), np.uint64), np.zeros((max(n, 1), 5), np.uint64), np.zeros(max(n, 1), np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib.pw_segment_last_plan_tables(vp(r), vp(s), vp(b), n)
    return r[:n].tolist(), s[:n].tolist(), b[:n].tolist()


def specialise_all(provers) -> int:
    """pw_provers_specialise: the run-time specialised kernels of all `provers` (Prover objects) in one concurrent compile batch,
    whatever their traces' heights. Returns how many run specialised kernels afterwards."""
    n = len(provers)
    arr = (C.c_void_p * max(n, 1))(*[p._h for p in provers])
    lib.pw_provers_specialise.restype = C.c_size_t
    lib.pw_provers_specialise.argtypes = [C.c_void_p, C.c_size_t]
    return int(lib.pw_provers_specialise(arr, n))


def set_device_budget(n_bytes: int) -> None:
    """pw_set_device_budget: bytes the provers of this process may plan for (0 = whatever the device has free)."""
    lib.pw_set_device_budget(int(n_bytes))


def verify_segment(descs, proof, num_queries: int = 100, pow_bits: int = 0, logup: bool = False, check_balance: bool = False,
                   preprocessed=None, transition: bool = False, public=None):
    """Host verification of a segment proof. descs: [(width, log_height, cons_bytecode, cons_spans, interactions-or-None)]
    -> (code, sum of the AIRs' cumulative bus sums). 0 = valid; ((i+1) << 8) | 2 = constraint identity of AIR i;
    14 = the bus sums do not cancel (check_balance); 16 = a preprocessed row does not open against its root.
    preprocessed: None (pw_verify_segment) or, per AIR, None | (width, root8) — the verifying key's preprocessed commitments
    (pw_verify_segment_preprocessed). transition: constraint operands over the row layout (RowOperands; pw_verify_segment_transition,
    which also takes `preprocessed`). public: None, or per AIR None (no public values) | an int (so many, accept what the proof
    carries) | the expected values (pw_verify_segment_public, DESIGN.md §5k: operands RowOperands.public(k); 17 = the proof's
    values differ from the expected ones)."""
    recs, keep = _air_descriptions(descs)
    pr = np.ascontiguousarray(proof, dtype=np.uint32)
    cfg = PwStarkConfig(num_queries, pow_bits)
    total = np.zeros(4, np.uint32)
    if public is not None:
        pre = _preprocessed_records(preprocessed, len(descs))
        pub, keep_pub = _public_records(public, len(descs))
        rc = int(lib.pw_verify_segment_public(C.byref(cfg), recs, pre, pub, len(descs), int(logup), _vp(pr), len(pr), int(check_balance), _vp(total)))
        return rc, total
    if transition and preprocessed is None:
        rc = int(lib.pw_verify_segment_transition(C.byref(cfg), recs, None, len(descs), int(logup), pr.ctypes.data_as(C.c_void_p), len(pr),
                                                  int(check_balance), total.ctypes.data_as(C.c_void_p)))
        return rc, total
    if preprocessed is None:
        rc = int(lib.pw_verify_segment(C.byref(cfg), recs, len(descs), int(logup), pr.ctypes.data_as(C.c_void_p), len(pr), int(check_balance),
                                       total.ctypes.data_as(C.c_void_p)))
        return rc, total
    assert len(preprocessed) == len(descs)
    pre = (PwAirPreprocessed * max(len(descs), 1))()
    for i, e in enumerate(preprocessed):
        if e is not None:
            w, root = e
            pre[i].width = int(w)
            for k, x in enumerate(np.asarray(root, dtype=np.uint32).reshape(8)):
                pre[i].root8[k] = int(x)
    fn = lib.pw_verify_segment_transition if transition else lib.pw_verify_segment_preprocessed
    rc = int(fn(C.byref(cfg), recs, pre, len(descs), int(logup), pr.ctypes.data_as(C.c_void_p), len(pr), int(check_balance),
                total.ctypes.data_as(C.c_void_p)))
    return rc, total


def _preprocessed_records(preprocessed, n: int):
    """per AIR None | (width, root8) -> PwAirPreprocessed[n], or None"""
    if preprocessed is None:
        return None
    assert len(preprocessed) == n
    pre = (PwAirPreprocessed * max(n, 1))()
    for i, e in enumerate(preprocessed):
        if e is not None:
            w, root = e
            pre[i].width = int(w)
            for k, x in enumerate(np.asarray(root, dtype=np.uint32).reshape(8)):
                pre[i].root8[k] = int(x)
    return pre


def _public_records(public, n: int):
    """per AIR None | count | expected values -> (PwAirPublic[n], the arrays its pointers point into)"""
    assert len(public) == n
    pub, keep = (PwAirPublic * max(n, 1))(), []
    for i, e in enumerate(public):
        if e is None:
            continue
        if isinstance(e, (int, np.integer)):
            pub[i].n = int(e)
            continue
        v = np.ascontiguousarray(e, dtype=np.uint32).reshape(-1)
        keep.append(v)
        pub[i].n, pub[i].expected = len(v), v.ctypes.data
    return pub, keep


def segment_public_values(descs, proof, public, air: int) -> np.ndarray:
    """pw_segment_proof_public_values: the public values AIR `air` carries in `proof` (canonical words). descs / public as for
    verify_segment (only the counts of `public` matter). Raises when the proof's header does not match; nothing else is checked."""
    recs, keep = _air_descriptions(descs)
    pub, keep_pub = _public_records(public, len(descs))
    pr = np.ascontiguousarray(proof, dtype=np.uint32)
    out = np.zeros(max(int(pub[air].n), 1), np.uint32)
    n = lib.pw_segment_proof_public_values(recs, pub, len(descs), _vp(pr), len(pr), air, _vp(out), len(out))
    if n == C.c_size_t(-1).value:
        raise ValueError("the proof's header does not match the descriptions")
    return out[:n].copy()


def verify_segment_chain(segments, links, num_queries: int = 100, pow_bits: int = 0):
    """pw_verify_segment_chain (host only): segments = [dict(descs, proof, public, preprocessed=None, logup=False, check_balance=False)]
    with the fields verify_segment takes; links = [(air_from, index_from, air_to, index_to)]: that public value of segment s equals this
    one of segment s + 1 (system_airs.connector_links). -> (code, where): 0; a segment's verifier code and its index; 18 and
    s * len(links) + link. That every segment ran the same program (the program AIR's preprocessed root) is the caller's to check."""
    n = len(segments)
    segs, keep = (PwChainSegment * max(n, 1))(), []
    for i, g in enumerate(segments):
        recs, k1 = _air_descriptions(g["descs"])
        pre = _preprocessed_records(g.get("preprocessed"), len(g["descs"]))
        pub, k2 = _public_records(g["public"], len(g["descs"])) if g.get("public") is not None else (None, [])
        pr = np.ascontiguousarray(g["proof"], dtype=np.uint32)
        keep += [recs, k1, pre, pub, k2, pr]
        segs[i] = PwChainSegment(recs, pre, pub, len(g["descs"]), int(g.get("logup", False)), pr.ctypes.data, len(pr), int(g.get("check_balance", False)))
    lk = (PwChainLink * max(len(links), 1))(*[PwChainLink(*[int(x) for x in l]) for l in links])
    cfg = PwStarkConfig(num_queries, pow_bits)
    where = C.c_size_t(0)
    rc = int(lib.pw_verify_segment_chain(C.byref(cfg), segs, n, lk, len(links), C.byref(where)))
    return rc, int(where.value)


def public_programs_check(width: int, cons_bytecode, cons_spans, n_public: int, interactions=None, pre_width: int = 0):
    """What Prover(..., n_public=) checks and compiles, without a GPU (test hook pw_public_programs_check): None when the entry would
    refuse the AIR, else dict(max_degree, row_flags, xbc: the constraints' xbc code, source: the generated HIP of the specialised
    quotient kernels — a function of the programs alone)."""
    bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
    sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
    tables, _ = _interaction_tables(interactions)
    deg, rf, nx, ns = C.c_int(), C.c_uint32(), C.c_size_t(), C.c_size_t()
    args = (width, pre_width, n_public, _vp(bc), len(bc), _vp(sp), len(sp), *tables, C.byref(deg), C.byref(rf))
    if lib.pw_public_programs_check(*args, None, 0, C.byref(nx), None, 0, C.byref(ns)) != 0:
        return None
    xbc, src = np.zeros(max(nx.value, 1), np.uint32), C.create_string_buffer(ns.value + 1)
    lib.pw_public_programs_check(*args, _vp(xbc), nx.value, C.byref(nx), src, ns.value + 1, C.byref(ns))
    return dict(max_degree=deg.value, row_flags=rf.value, xbc=xbc[:nx.value].copy(), source=src.value.decode())


def verify_airs(descs, proofs, num_queries: int = 100, pow_bits: int = 0, shared_bus_seed: bool = False, check_balance: bool = False):
    """descs: [(width, log_height, cons_bytecode, cons_spans, interactions-or-None)] -> (code, total bus sum).
    code 0 = every proof valid (and balanced if asked); ((i+1) << 8) | c = proof i failed check c; 14 = unbalanced."""
    n = len(descs)
    recs, keep = _air_descriptions(descs)
    prs = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
    ptrs = (C.c_void_p * max(n, 1))(*[p.ctypes.data for p in prs])
    lens = (C.c_size_t * max(n, 1))(*[len(p) for p in prs])
    cfg = PwStarkConfig(num_queries, pow_bits)
    total = np.zeros(4, np.uint32)
    rc = int(lib.pw_verify_airs(C.byref(cfg), recs, n, ptrs, lens, int(shared_bus_seed), int(check_balance), _vp(total)))
    return rc, total


def poseidon2_host(state) -> np.ndarray:
    s = np.ascontiguousarray(state, dtype=np.uint32).copy()
    lib.pw_poseidon2_permute_host(s.ctypes.data_as(C.c_void_p))
    return s


lib.pw_set_poseidon2_constants.restype = C.c_int
lib.pw_set_poseidon2_constants.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_get_poseidon2_constants.restype = None
lib.pw_get_poseidon2_constants.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]


def jit_compile_check(width: int, cons_bytecode, cons_spans, interactions=None) -> dict:
    """pw_jit_compile_check: generate + compile the specialised kernels of an AIR on the host (no GPU needed)."""
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
    sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
    k, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    err = C.create_string_buffer(4096)
    f = lib.pw_jit_compile_check
    f.restype = C.c_int
    f.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                  C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    tables, _ = _interaction_tables(interactions)
    rc = f(width, vp(bc), len(bc), vp(sp), len(sp), *tables, C.byref(k), C.byref(b), C.byref(c), err, 4096)
    return dict(rc=int(rc), kernels=k.value, code_bytes=b.value, chunks=c.value, error=err.value.decode(errors="replace"))


def jit_generated_sources(width: int, cons_bytecode, cons_spans, interactions=None, which: int = 0, chunk_cost: int = 0, chunks_per_unit: int = 0):
    """pw_jit_generated_source for every translation unit: ([{source, kernel, first_chunk, n_chunks}], total chunks). which: 0 = the
    quotient numerator, 1 = the LogUp permutation columns. No compilation, no GPU (a test hook)."""
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
    sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
    f = lib.pw_jit_generated_source
    f.restype = C.c_size_t
    f.argtypes = [C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                  C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint32),
                  C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    tables, _ = _interaction_tables(interactions)
    units, total = [], C.c_uint32()
    while True:
        first, n, name = C.c_uint32(), C.c_uint32(), C.create_string_buffer(64)
        size = f(width, vp(bc), len(bc), vp(sp), len(sp), *tables, which, chunk_cost, chunks_per_unit, len(units), None, 0, name, 64, C.byref(first), C.byref(n),
                 C.byref(total))
        if size == 0:
            break
        buf = C.create_string_buffer(size + 1)
        f(width, vp(bc), len(bc), vp(sp), len(sp), *tables, which, chunk_cost, chunks_per_unit, len(units), buf, size + 1, name, 64, C.byref(first), C.byref(n),
          C.byref(total))
        units.append(dict(source=buf.value.decode(), kernel=name.value.decode(), first_chunk=first.value, n_chunks=n.value))
    return units, total.value


def jit_cache_stats() -> dict:
    """pw_jit_cache_stats: translation units this process compiled / loaded from the on-disk code-object cache."""
    lib.pw_jit_cache_stats.restype = None
    lib.pw_jit_cache_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    a, b = C.c_uint64(), C.c_uint64()
    lib.pw_jit_cache_stats(C.byref(a), C.byref(b))
    return dict(compiled=a.value, from_disk=b.value)


_SEGMENT_PROVE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.POINTER(C.c_uint32))
lib.pw_prove_segments_multi.restype = C.c_int
lib.pw_prove_segments_multi.argtypes = [C.POINTER(C.c_int), C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, _SEGMENT_PROVE_FN, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
lib.pw_multi_last_merge.restype = C.c_int
lib.pw_assign_units.restype = C.c_size_t
lib.pw_assign_units.argtypes = [C.POINTER(C.c_uint64), C.c_size_t, C.c_size_t, C.c_void_p]


def assign_units(cells, n_workers: int) -> np.ndarray:
    """pw_assign_units: worker of every unit (largest first, each to the least loaded worker)."""
    n = len(cells)
    out = np.zeros(n, np.uint32)
    arr = (C.c_uint64 * max(n, 1))(*[int(c) for c in cells])
    assert lib.pw_assign_units(arr, n, n_workers, out.ctypes.data_as(C.c_void_p)) == n
    return out


def prove_segments_multi(devices, segment_cells, prove_segment):
    """pw_prove_segments_multi: one host thread per entry of `devices` proves the segments placed on it by calling
    prove_segment(segment, worker, device) -> 8 commitment words; the commitments are merged over RCCL.
    Returns (uint32 [n_segments, 8], worker of every segment, merge kind: 1 = RCCL all-gather, 2 = host)."""
    n = len(segment_cells)
    errors = []

    def cb(_user, segment, worker, device, out):
        try:
            c = np.asarray(prove_segment(int(segment), int(worker), int(device)), dtype=np.uint32).reshape(8)
            for i in range(8):
                out[i] = int(c[i])
            return 0
        except Exception as e:  # noqa: BLE001 - reported to the caller below
            errors.append(e)
            return 1

    fn = _SEGMENT_PROVE_FN(cb)
    devs = (C.c_int * len(devices))(*[int(d) for d in devices])
    cells = (C.c_uint64 * max(n, 1))(*[int(c) for c in segment_cells])
    commitments = np.zeros((n, 8), np.uint32)
    owner = np.zeros(n, np.uint32)
    rc = lib.pw_prove_segments_multi(devs, len(devices), cells, n, fn, None, commitments.ctypes.data_as(C.c_void_p), owner.ctypes.data_as(C.c_void_p))
    if errors:
        raise errors[0]
    abi.check(rc, "pw_prove_segments_multi")
    return commitments, owner, int(lib.pw_multi_last_merge())


def set_poseidon2_constants(ext_rc=None, int_rc=None) -> None:
    """pw_set_poseidon2_constants: 8 x 16 external + 13 internal round constants (canonical); None, None = the placeholder."""
    if ext_rc is None:
        rc = lib.pw_set_poseidon2_constants(None, None)
    else:
        e = np.ascontiguousarray(ext_rc, dtype=np.uint32).reshape(8, 16)
        i = np.ascontiguousarray(int_rc, dtype=np.uint32).reshape(13)
        rc = lib.pw_set_poseidon2_constants(e.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p))
    if rc:
        raise ValueError("round constants must be canonical field elements")


def poseidon2_constants():
    e, i, d = np.zeros((8, 16), np.uint32), np.zeros(13, np.uint32), np.zeros(16, np.uint32)
    lib.pw_get_poseidon2_constants(e.ctypes.data_as(C.c_void_p), i.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p))
    return e, i, d


lib.powdr_poseidon2_derived.restype = C.c_size_t
lib.powdr_poseidon2_derived.argtypes = [C.c_void_p, C.c_size_t]


def poseidon2_derived() -> dict:
    """powdr_poseidon2_derived (a read-only test hook): the derived tables of the installed table as Python integers."""
    v = np.zeros(194, np.int64)
    assert lib.powdr_poseidon2_derived(v.ctypes.data_as(C.c_void_p), len(v)) == len(v)
    v = [int(x) for x in v]
    return dict(ext_fold=[v[16 * r:16 * r + 16] for r in range(8)], entry_c=v[128], part_kappa=v[129:131], part_rho=v[131:133],
                part_diag=[v[133:149], v[149:165]], int_fold=v[165:178], exit_fold=v[178:194])


class Prover:
    """One AIR = one prover (constraint programs fixed at construction).

    interactions = (inter[n x 3] = {bus, n_args, first span}, spans[m x 2], bytecode) — the output of
    host.compile_bus(apc, 1) — switches the prover to "pw-stark v0 + LogUp" (proof magic PWS2).

    preprocessed = (device tensor of the fixed matrix (column-major, Montgomery), pre_width, log_height): operands width ..
    width + pre_width - 1 of the programs are those columns (pw_prover_create_preprocessed; segment proofs only, at that height).

    transition = True: the constraint programs may read the next row and the row selectors (RowOperands, DESIGN.md §5h;
    pw_prover_create_transition, with or without `preprocessed`; segment proofs only).

    n_public > 0: the AIR has that many public values (RowOperands.public(k); pw_prover_create_public, with or without
    `preprocessed` and next-row reads; segment proofs only): set_public_values before every segment proof whose values differ."""

    def __init__(self, width: int, cons_bytecode, cons_spans, num_queries: int = 100, pow_bits: int = 0, interactions=None,
                 preprocessed=None, transition: bool = False, n_public: int = 0):
        bc = np.ascontiguousarray(cons_bytecode, dtype=np.uint32)
        sp = np.ascontiguousarray(cons_spans, dtype=np.uint32).reshape(-1, 2)
        cfg = PwStarkConfig(num_queries, pow_bits)
        self.width = width
        self.pre_width = 0
        self.n_public = int(n_public)
        tables, _ = _interaction_tables(interactions)
        if n_public:
            t, pw_, lh = preprocessed if preprocessed is not None else (None, 0, 0)
            if t is not None:
                assert t.numel() == pw_ << lh, "the fixed matrix must hold pre_width x 2^log_height words"
            self._h = lib.pw_prover_create_public(C.byref(cfg), width, pw_, lh, t.data_ptr() if t is not None else None, int(n_public), _vp(bc), len(bc),
                                                  _vp(sp), len(sp), *tables)
            self.pre_width = pw_
        elif transition or preprocessed is not None:
            t, pw_, lh = preprocessed if preprocessed is not None else (None, 0, 0)
            if t is not None:
                assert t.numel() == pw_ << lh, "the fixed matrix must hold pre_width x 2^log_height words"
            create = lib.pw_prover_create_transition if transition else lib.pw_prover_create_preprocessed
            self._h = create(C.byref(cfg), width, pw_, lh, t.data_ptr() if t is not None else None, _vp(bc), len(bc), _vp(sp), len(sp), *tables)
            self.pre_width = pw_
        elif interactions is None:
            self._h = lib.pw_prover_create(C.byref(cfg), width, _vp(bc), len(bc), _vp(sp), len(sp))
        else:
            self._h = lib.pw_prover_create_logup(C.byref(cfg), width, _vp(bc), len(bc), _vp(sp), len(sp), *tables)
        if not self._h:
            raise RuntimeError("pw_prover_create failed")

    @property
    def row_flags(self) -> int:
        """pw_prover_row_flags: bit 0 the constraints read a next-row operand, bit 1 a row selector (0: not row-aware)."""
        return int(lib.pw_prover_row_flags(self._h))

    def set_public_values(self, values) -> None:
        """pw_prover_set_public_values: n_public canonical words (the prover keeps a copy; a segment proof snapshots them when it begins)."""
        v = np.ascontiguousarray(values, dtype=np.uint32).reshape(-1)
        if lib.pw_prover_set_public_values(self._h, _vp(v), len(v)) != 0:
            raise ValueError(f"{len(v)} public values for an AIR with {self.n_public}, or a word that is no canonical field element")

    def preprocessed_root(self) -> np.ndarray:
        """pw_prover_preprocessed_root: the commitment to the fixed matrix (8 canonical words; the verifying key's part)."""
        root = np.zeros(8, np.uint32)
        abi.check(lib.pw_prover_preprocessed_root(self._h, root.ctypes.data_as(C.c_void_p)), "pw_prover_preprocessed_root")
        return root

    def prove(self, d_trace_ptr: int, log_height: int, copy: bool = True, consume: bool = False) -> np.ndarray:
        """pw_prover_prove; consume=True: pw_prover_prove_consuming — the trace is handed over (a streamed proof leaves its
        coefficient arrays there: trace_from_coefficients restores it)."""
        words = C.POINTER(C.c_uint32)()
        n = C.c_size_t()
        fn = lib.pw_prover_prove_consuming if consume else lib.pw_prover_prove
        rc = fn(self._h, d_trace_ptr, log_height, C.byref(words), C.byref(n))
        abi.check(rc, "pw_prover_prove_consuming" if consume else "pw_prover_prove")
        a = np.ctypeslib.as_array(words, shape=(n.value,))
        return a.copy() if copy else a

    def trace_root(self, d_trace_ptr: int, log_height: int) -> np.ndarray:
        """Commitment to the trace alone (8 canonical words) — phase 1 of a multi-AIR LogUp segment."""
        root = np.zeros(8, np.uint32)
        abi.check(lib.pw_prover_trace_root(self._h, d_trace_ptr, log_height, root.ctypes.data_as(C.c_void_p)), "pw_prover_trace_root")
        return root

    def set_bus_seed(self, seed) -> None:
        """Seed of the bus challenges shared by all AIRs of a segment (None: back to the AIR's own trace root)."""
        a = None if seed is None else np.ascontiguousarray(seed, dtype=np.uint32)
        abi.check(lib.pw_prover_set_bus_seed(self._h, None if a is None else a.ctypes.data_as(C.c_void_p)), "pw_prover_set_bus_seed")

    def check_constraints(self, d_trace_ptr: int, log_height: int):
        """Mock prover: (number of violated (row, constraint) pairs, first row, first constraint)."""
        n, row, c = C.c_uint64(), C.c_uint64(), C.c_uint32()
        rc = lib.pw_prover_check_constraints(self._h, d_trace_ptr, log_height, C.byref(n), C.byref(row), C.byref(c))
        abi.check(rc, "pw_prover_check_constraints")
        return (n.value, row.value, c.value) if n.value else (0, None, None)

    def reserve(self, log_height: int) -> None:
        """Allocate the device buffers of a 2^log_height-row proof now (the first prove otherwise pays for it)."""
        lib.pw_prover_reserve.restype = C.c_int
        lib.pw_prover_reserve.argtypes = [C.c_void_p, C.c_uint32]
        abi.check(lib.pw_prover_reserve(self._h, log_height), "pw_prover_reserve")

    def stream_log_blocks(self, log_height: int) -> int:
        """pw_prover_stream_log_blocks: 0 = a proof of this height keeps the LDE resident, b >= 1 = streamed over 2^b sub-cosets of
        the extended domain (the memory free now decides; POWDR_STREAM_LOG_BLOCKS forces), -1 = does not fit."""
        lib.pw_prover_stream_log_blocks.restype = C.c_int
        lib.pw_prover_stream_log_blocks.argtypes = [C.c_void_p, C.c_uint32]
        return int(lib.pw_prover_stream_log_blocks(self._h, log_height))

    def stream_log_blocks_consuming(self, log_height: int) -> int:
        """the same for prove(..., consume=True): the trace's coefficients need no buffer of their own"""
        return int(lib.pw_prover_stream_log_blocks_consuming(self._h, log_height))

    def specialise(self) -> bool:
        """pw_prover_specialise: compile the run-time specialised kernels now. True if the prover has them."""
        lib.pw_prover_specialise.restype = C.c_int
        lib.pw_prover_specialise.argtypes = [C.c_void_p]
        return int(lib.pw_prover_specialise(self._h)) == 0

    def specialised(self) -> dict:
        """pw_prover_specialised: {"state": 1 specialised | 0 not tried | -1 interpreter only, "kernels", "code_bytes", "chunks"}."""
        lib.pw_prover_specialised.restype = C.c_int
        lib.pw_prover_specialised.argtypes = [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        k, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        st = int(lib.pw_prover_specialised(self._h, C.byref(k), C.byref(b), C.byref(c)))
        return dict(state=st, kernels=k.value, code_bytes=b.value, chunks=c.value)

    def quotient_units(self):
        """[(g0, g1)] per translation unit of the specialised quotient kernels: the LogUp groups the unit reads (pw_prover_quotient_units,
        pw_prover_quotient_unit_groups); [] for a prover that is not specialised."""
        out = []
        for u in range(int(lib.pw_prover_quotient_units(self._h))):
            g0, g1 = C.c_uint32(), C.c_uint32()
            abi.check(lib.pw_prover_quotient_unit_groups(self._h, u, C.byref(g0), C.byref(g1)), "pw_prover_quotient_unit_groups")
            out.append((g0.value, g1.value))
        return out

    def max_constraint_degree(self) -> int:
        lib.pw_prover_max_constraint_degree.restype = C.c_int
        lib.pw_prover_max_constraint_degree.argtypes = [C.c_void_p]
        return int(lib.pw_prover_max_constraint_degree(self._h))

    def device_bytes(self) -> int:
        return int(lib.pw_prover_device_bytes(self._h))

    def logup_path(self) -> int:
        """0 = no LogUp extension, 1 = interpreter, 2 = small forms (pw_prover_logup_path)."""
        return int(lib.pw_prover_logup_path(self._h))

    def close(self):
        if self._h:
            lib.pw_prover_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def trace_from_coefficients(d_ptr: int, width: int, log_height: int) -> None:
    """pw_trace_from_coefficients, in place: what a streamed consuming proof left in the caller's trace buffer -> the trace."""
    import torch

    scratch = torch.empty(1 << 13, dtype=torch.int32, device="cuda")
    abi.check(lib.pw_trace_from_coefficients(d_ptr, width, log_height, scratch.data_ptr()), "pw_trace_from_coefficients")
    torch.cuda.synchronize()  # (the scratch goes out of scope)
