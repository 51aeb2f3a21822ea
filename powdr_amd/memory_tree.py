"""The sparse memory Merkle tree on the device (include/powdr_prover.h `pw_memory_tree_*`): a binary Poseidon2 tree over
2^height leaves of 8 words that lives from segment to segment — its roots before and after a segment, the check that a segment starts
from the memory the last one left, and the opened paths as (left, right, out) rows the Poseidon2 chip receives on BUS_COMPRESS.

  MemoryTree(height=30)   load(keys, payloads) an initial image; update(keys, init, fin) one segment's touched leaves; root(); stats()
                          incremental=True (or the `incremental` property, between any two updates): an update hashes only the touched
                          paths and moves every other stored node, instead of hashing every level again — the same bytes either way
  boundary_leaves         keys and payloads of the rows of a memory boundary trace (key = (as - 1) * 2^29 + ptr)
  records_air             the sender of the records: 25 columns [valid, left[8], right[8], out[8]]

Nothing in a proof constrains the records yet beyond "each is a compression": the Merkle AIR and the persistent boundary AIR come next.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi
from .periphery import _col, _tables
from .periphery import OP_PUSH_APC, OP_PUSH_CONST
from .system_airs import BUS_COMPRESS, OP_MUL, OP_SUB, SystemAir, _to_monty

lib = abi.lib


class PwMemoryTreeStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("leaves", "stored_nodes", "device_bytes", "last_permutations", "last_launches", "last_scratch_bytes")]


lib.pw_memory_tree_create.restype = C.c_void_p
lib.pw_memory_tree_create.argtypes = [C.c_uint32]
lib.pw_memory_tree_destroy.restype = None
lib.pw_memory_tree_destroy.argtypes = [C.c_void_p]
lib.pw_memory_tree_root.restype = C.c_int
lib.pw_memory_tree_root.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_memory_tree_stats.restype = C.c_int
lib.pw_memory_tree_stats.argtypes = [C.c_void_p, C.POINTER(PwMemoryTreeStats)]
lib.pw_memory_tree_update.restype = C.c_int
lib.pw_memory_tree_update.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint32,
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
lib.pw_memory_tree_boundary_leaves.restype = C.c_int
lib.pw_memory_tree_boundary_leaves.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]

lib.pw_memory_tree_set_mode.restype = C.c_int
lib.pw_memory_tree_set_mode.argtypes = [C.c_void_p, C.c_uint32]
lib.pw_memory_tree_get_mode.restype = C.c_int
lib.pw_memory_tree_get_mode.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]

MODE_REBUILD, MODE_INCREMENTAL = 0, 1  # PW_MEMORY_TREE_REBUILD, PW_MEMORY_TREE_INCREMENTAL
TAIL_NODES = 1024  # csrc/memory_tree.hip kMemoryTreeTailNodes: a level of at most this many nodes is finished by one workgroup
RECORD_WIDTH = 25
RECORD_COLUMNS = ["valid"] + [f"left{i}" for i in range(8)] + [f"right{i}" for i in range(8)] + [f"out{i}" for i in range(8)]
STATUS = {0: "updated", 1: "cap_log_height too small", 3: "init is not what the tree holds", 4: "keys not strictly increasing or out of range",
          5: "a payload word that is no field element"}


def _keys(keys) -> torch.Tensor:
    """leaf indices on the device: a device int64 tensor as it is, anything else through numpy uint64"""
    if isinstance(keys, torch.Tensor):
        assert keys.dtype == torch.int64 and keys.is_cuda and keys.is_contiguous()
        return keys
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64).reshape(-1)).cuda()


def _payloads(words, n: int) -> torch.Tensor:
    """[n, 8] words on the device in Montgomery form: a device int32 tensor is taken to hold Montgomery words already, anything else
    canonical words"""
    if isinstance(words, torch.Tensor):
        assert words.dtype == torch.int32 and words.is_cuda and words.is_contiguous() and words.numel() == 8 * n
        return words
    a = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    assert a.size == 8 * n and (a < 0x78000001).all(), "payloads are n x 8 canonical words"
    return torch.from_numpy(_to_monty(a).view(np.int32)).cuda()


class MemoryTree:
    """pw_memory_tree_create .. pw_memory_tree_destroy. Keys: increasing leaf indices below 2^height (numpy / list, or a device int64
    tensor); payloads: [n, 8] canonical words (numpy / list), or a device int32 tensor of Montgomery words. The tree belongs to the
    Poseidon2 table installed when it is made: under another table every call raises. incremental: pw_memory_tree_set_mode — updates
    hash only the touched paths (load() is the full rebuild either way); may be changed between any two updates."""

    def __init__(self, height: int = 30, incremental: bool = False):
        self._h = lib.pw_memory_tree_create(int(height))
        if not self._h:
            raise ValueError("the height of a memory tree is 1 .. 40")
        self.height = int(height)
        if incremental:
            self.incremental = True

    @property
    def incremental(self) -> bool:
        mode = C.c_uint32()
        abi.check(lib.pw_memory_tree_get_mode(self._h, C.byref(mode)), "pw_memory_tree_get_mode")
        return mode.value == MODE_INCREMENTAL

    @incremental.setter
    def incremental(self, on: bool) -> None:
        abi.check(lib.pw_memory_tree_set_mode(self._h, MODE_INCREMENTAL if on else MODE_REBUILD), "pw_memory_tree_set_mode")

    def close(self) -> None:
        if getattr(self, "_h", None) and lib is not None:
            lib.pw_memory_tree_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def root(self) -> np.ndarray:
        """the root as 8 canonical words"""
        out = np.zeros(8, np.uint32)
        abi.check(lib.pw_memory_tree_root(self._h, out.ctypes.data_as(C.c_void_p)), "pw_memory_tree_root")
        return out

    def stats(self) -> dict:
        st = PwMemoryTreeStats()
        abi.check(lib.pw_memory_tree_stats(self._h, C.byref(st)), "pw_memory_tree_stats")
        return {n: int(getattr(st, n)) for n, _ in PwMemoryTreeStats._fields_}

    def load(self, keys, payloads):
        """load mode: the payloads are written, whatever the leaves held -> (status, info): 0, or 4 / 5 with the offending index"""
        k = _keys(keys)
        p = _payloads(payloads, k.numel())
        torch.cuda.synchronize()
        status, info = C.c_uint32(), C.c_uint64()
        abi.check(lib.pw_memory_tree_update(self._h, k.data_ptr(), None, p.data_ptr(), k.numel(), None, None, 0, None, None, C.byref(status), C.byref(info)),
                  "pw_memory_tree_update")
        return int(status.value), int(info.value)

    def update(self, keys, init, fin, records: bool = True, cap_log_height: int = 10, out: torch.Tensor | None = None, node_ids: bool = False):
        """One segment: every key must hold `init` (the zero payload: not stored) and holds `fin` afterwards -> (status, info, records
        trace, log_h, n_rows): status a key of STATUS, info the smallest mismatching key (3) or the first offending index (4, 5); the
        trace = 25 x 2^log_h Montgomery words, column-major (RECORD_COLUMNS) — None without records or with a non-zero status. Status 1
        is retried once at the height the library asked for, in a buffer of that height — unless the caller gave `out`, whose size is
        the caller's business. node_ids: the trace comes as (trace, ids), ids = one int64 per row (phase << 63 | level << 56 | index).
        With a non-zero status the tree is what it was."""
        k = _keys(keys)
        n = k.numel()
        a, b = _payloads(init, n), _payloads(fin, n)
        torch.cuda.synchronize()
        own = out is None
        for _ in range(2):
            ids = None
            if records:
                if own:
                    out = torch.empty(RECORD_WIDTH << cap_log_height, dtype=torch.int32, device="cuda")
                assert out.numel() >= RECORD_WIDTH << cap_log_height
                if node_ids:
                    ids = torch.zeros(1 << cap_log_height, dtype=torch.int64, device="cuda")
            lh, rows, status, info = C.c_uint32(), C.c_uint64(), C.c_uint32(), C.c_uint64()
            abi.check(lib.pw_memory_tree_update(self._h, k.data_ptr(), a.data_ptr(), b.data_ptr(), n, out.data_ptr() if records else None,
                                                ids.data_ptr() if ids is not None else None, cap_log_height, C.byref(lh), C.byref(rows), C.byref(status),
                                                C.byref(info)), "pw_memory_tree_update")
            if status.value != 1 or not own:
                break
            cap_log_height = int(lh.value)
        trace = None
        if records and status.value == 0:
            trace = out[:RECORD_WIDTH << lh.value]
            if node_ids:
                trace = (trace, ids[:int(rows.value)])
        return int(status.value), int(info.value), trace, int(lh.value), int(rows.value)


def boundary_leaves(trace: torch.Tensor, log_h: int, n_locations: int):
    """pw_memory_tree_boundary_leaves: a memory boundary trace (system_airs.memory_boundary_trace) -> (keys: device int64 [n], init, fin:
    device int32 [n, 8] Montgomery words) — what MemoryTree.update takes"""
    n = int(n_locations)
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    init = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    fin = torch.empty((n, 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    abi.check(lib.pw_memory_tree_boundary_leaves(trace.data_ptr(), int(log_h), n, keys.data_ptr(), init.data_ptr(), fin.data_ptr()),
              "pw_memory_tree_boundary_leaves")
    return keys, init, fin


def records_air(bus: int = BUS_COMPRESS) -> SystemAir:
    """The records as an AIR: 25 main columns RECORD_COLUMNS, one constraint valid (valid - 1), and one interaction that sends
    (left, right, out) on `bus` with multiplicity valid — the first sender on the compression bus in the product."""
    cons = (np.array([OP_PUSH_APC, 0, OP_PUSH_APC, 0, OP_PUSH_CONST, 1, OP_SUB, OP_MUL], np.uint32), np.array([[0, 8]], np.uint32))
    inter = _tables(bus, [(_col(0), [_col(1 + j) for j in range(24)])])
    return SystemAir("memory_records", RECORD_WIDTH, cons, inter, list(RECORD_COLUMNS))
