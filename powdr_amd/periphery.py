"""The receive side of the lookup buses: traces of the shared periphery chips from the histograms
`_apc_apply_bus` fills (include/powdr_gpu.h `powdr_periphery_*_trace`) and the bus interactions those
AIRs declare, in the table format of `pw_prover_create_logup` / `host.Apc.compile_bus(1)`.

The chips are external to the reference repository (openvm-circuit-primitives; instantiated in
openvm/src/powdr_extension/trace_generator/cuda/periphery.rs:33-85); the tuple <-> histogram index maps are
the reference's (openvm/cuda/src/apc_apply_bus.cu:74,89,104)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi

lib = abi.lib
PERIPHERY_SYMBOLS = ["powdr_periphery_var_range_trace", "powdr_periphery_tuple2_trace", "powdr_periphery_bitwise_trace",
                     "powdr_periphery_var_range_table", "powdr_periphery_tuple2_table", "powdr_periphery_bitwise_table",
                     "powdr_periphery_multiplicities"]
lib.powdr_periphery_var_range_trace.restype = C.c_int
lib.powdr_periphery_var_range_trace.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
lib.powdr_periphery_tuple2_trace.restype = C.c_int
lib.powdr_periphery_tuple2_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.powdr_periphery_bitwise_trace.restype = C.c_int
lib.powdr_periphery_bitwise_trace.argtypes = [C.c_void_p, C.c_void_p]
lib.powdr_periphery_var_range_table.restype = C.c_int
lib.powdr_periphery_var_range_table.argtypes = [C.c_size_t, C.c_void_p]
lib.powdr_periphery_tuple2_table.restype = C.c_int
lib.powdr_periphery_tuple2_table.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
lib.powdr_periphery_bitwise_table.restype = C.c_int
lib.powdr_periphery_bitwise_table.argtypes = [C.c_void_p]
lib.powdr_periphery_multiplicities.restype = C.c_int
lib.powdr_periphery_multiplicities.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]

OP_PUSH_APC, OP_PUSH_CONST, OP_NEG = 0, 1, 5


def var_range_trace(hist: torch.Tensor) -> torch.Tensor:
    """[value, bits, mult] x len(hist) rows, column-major, Montgomery."""
    out = torch.empty(3 * hist.numel(), dtype=torch.int32, device=hist.device)
    abi.check(lib.powdr_periphery_var_range_trace(hist.data_ptr(), hist.numel(), out.data_ptr()), "powdr_periphery_var_range_trace")
    return out


def tuple2_trace(hist: torch.Tensor, sizes) -> torch.Tensor:
    """[v0, v1, mult] x sz0*sz1 rows."""
    out = torch.empty(3 * hist.numel(), dtype=torch.int32, device=hist.device)
    assert hist.numel() == sizes[0] * sizes[1]
    abi.check(lib.powdr_periphery_tuple2_trace(hist.data_ptr(), sizes[0], sizes[1], out.data_ptr()), "powdr_periphery_tuple2_trace")
    return out


def bitwise_trace(hist: torch.Tensor) -> torch.Tensor:
    """[x, y, x^y, mult_range, mult_xor] x 65 536 rows from the [range | xor] histogram."""
    assert hist.numel() == 2 * 65536
    out = torch.empty(5 * 65536, dtype=torch.int32, device=hist.device)
    abi.check(lib.powdr_periphery_bitwise_trace(hist.data_ptr(), out.data_ptr()), "powdr_periphery_bitwise_trace")
    return out


# ---- the chips' own layout: the tuples in preprocessed columns (fixed by the proving key), the multiplicities in the main trace ----
def var_range_table(n_bins: int, device="cuda") -> torch.Tensor:
    """[value, bits] x n_bins rows: the var-range AIR's preprocessed matrix."""
    out = torch.empty(2 * n_bins, dtype=torch.int32, device=device)
    abi.check(lib.powdr_periphery_var_range_table(n_bins, out.data_ptr()), "powdr_periphery_var_range_table")
    return out


def tuple2_table(sizes, device="cuda") -> torch.Tensor:
    """[v0, v1] x sz0*sz1 rows."""
    out = torch.empty(2 * sizes[0] * sizes[1], dtype=torch.int32, device=device)
    abi.check(lib.powdr_periphery_tuple2_table(sizes[0], sizes[1], out.data_ptr()), "powdr_periphery_tuple2_table")
    return out


def bitwise_table(device="cuda") -> torch.Tensor:
    """[x, y, x^y] x 65 536 rows."""
    out = torch.empty(3 * 65536, dtype=torch.int32, device=device)
    abi.check(lib.powdr_periphery_bitwise_table(out.data_ptr()), "powdr_periphery_bitwise_table")
    return out


def multiplicities(hist: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """hist mod p in Montgomery form: the main trace of a periphery AIR in the preprocessed layout (for bitwise the [range | xor]
    histogram is the two columns [mult_range, mult_xor])."""
    if out is None:
        out = torch.empty(hist.numel(), dtype=torch.int32, device=hist.device)
    assert out.numel() >= hist.numel()
    abi.check(lib.powdr_periphery_multiplicities(hist.data_ptr(), hist.numel(), out.data_ptr()), "powdr_periphery_multiplicities")
    return out


def _tables(bus: int, rows):
    """rows: list of (mult program, [arg programs]) -> (interactions[n,3], spans[m,2], bytecode)"""
    inter, spans, bc = [], [], []
    for mult, args in rows:
        inter.append((bus, len(args), len(spans)))
        for prog in [mult] + args:
            spans.append((len(bc), len(prog)))
            bc += prog
    return np.array(inter, np.uint32).reshape(-1, 3), np.array(spans, np.uint32).reshape(-1, 2), np.array(bc, np.uint32)


def _join_tables(by_bus):
    """[(bus, rows of _tables)] -> one interaction table over the buses: spans and bytecode concatenated"""
    inter, ispans, ibc = [], [], []
    for bus, rows_ in by_bus:
        it, sp, code = _tables(bus, rows_)
        it = it.copy()
        it[:, 2] += len(ispans)
        sp = sp.copy()
        sp[:, 0] += len(ibc)
        inter += it.tolist()
        ispans += sp.tolist()
        ibc += code.tolist()
    return np.array(inter, np.uint32).reshape(-1, 3), np.array(ispans, np.uint32).reshape(-1, 2), np.array(ibc, np.uint32)


def _col(c):
    return [OP_PUSH_APC, c]


def _neg_col(c):
    return [OP_PUSH_APC, c, OP_NEG]


def var_range_interactions(bus: int = 3):
    """receive (value, bits) `mult` times"""
    return _tables(bus, [(_neg_col(2), [_col(0), _col(1)])])


def tuple2_interactions(bus: int = 7):
    return _tables(bus, [(_neg_col(2), [_col(0), _col(1)])])


def bitwise_interactions(bus: int = 6):
    """receive (x, y, 0, 0) `mult_range` times and (x, y, x^y, 1) `mult_xor` times"""
    return _tables(bus, [(_neg_col(3), [_col(0), _col(1), [OP_PUSH_CONST, 0], [OP_PUSH_CONST, 0]]),
                         (_neg_col(4), [_col(0), _col(1), _col(2), [OP_PUSH_CONST, 1]])])


# operands of the preprocessed layout: main columns first (the multiplicities), then the fixed ones (pw_prover_create_preprocessed)
def var_range_interactions_pre(bus: int = 3):
    """main [mult] | pre [value, bits]: receive (value, bits) `mult` times"""
    return _tables(bus, [(_neg_col(0), [_col(1), _col(2)])])


def tuple2_interactions_pre(bus: int = 7):
    """main [mult] | pre [v0, v1]"""
    return _tables(bus, [(_neg_col(0), [_col(1), _col(2)])])


def bitwise_interactions_pre(bus: int = 6):
    """main [mult_range, mult_xor] | pre [x, y, x^y]"""
    return _tables(bus, [(_neg_col(0), [_col(2), _col(3), [OP_PUSH_CONST, 0], [OP_PUSH_CONST, 0]]),
                         (_neg_col(1), [_col(2), _col(3), _col(4), [OP_PUSH_CONST, 1]])])


def select_buses(interactions, buses):
    """Restrict an interaction table (interactions, spans, bytecode) to the given bus ids (spans and bytecode are
    kept whole; only the interaction rows are filtered)."""
    inter, spans, bc = interactions
    inter = np.asarray(inter, np.uint32).reshape(-1, 3)
    keep = np.isin(inter[:, 0], np.asarray(list(buses), np.uint32))
    return np.ascontiguousarray(inter[keep]), spans, bc
