"""Empirical constraints (include/powdr_prover.h `pw_empirical_detect`): what the reference's
`detect_empirical_constraints` computes from the instruction chips' traces — per executed pc the 1st and 99th percentile of every
column, per basic block the partition of its cells into classes that held equal values in every execution of the block — found on
the device, and the reference's `EmpiricalConstraints` with its host-side semantics (`combine_with`, `apply_pc_threshold`) and the
JSON layout serde gives it, so that `to_json()` is the `empirical_constraints.json` its `compile_apcs` reads.

Basic blocks come from the caller (the reference's `collect_basic_blocks`, or a candidates file)."""
from __future__ import annotations

import ctypes as C
import json
from dataclasses import dataclass, field

import numpy as np

from . import abi, prover, stage

lib = abi.lib
BUS_EXEC = 0
STATUS = {0: "found", **stage.texts(2, 3, 4, 6, 7), 5: "a pc executed by two AIRs"}


class PwBasicBlock(C.Structure):
    _fields_ = [("start_pc", C.c_uint32), ("n_instructions", C.c_uint32)]


_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
lib.pw_empirical_detect.restype = C.c_int
lib.pw_empirical_detect.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(PwBasicBlock), C.c_size_t, C.c_size_t,
                                    C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_empirical_destroy.restype = None
lib.pw_empirical_destroy.argtypes = [C.c_void_p]
lib.pw_empirical_sizes.restype = None
lib.pw_empirical_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_empirical_read_pcs.restype = None
lib.pw_empirical_read_pcs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_empirical_read_ranges.restype = None
lib.pw_empirical_read_ranges.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_empirical_read_blocks.restype = None
lib.pw_empirical_read_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_empirical_read_cells.restype = None
lib.pw_empirical_read_cells.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_empirical_percentile_indices.restype = None
lib.pw_empirical_percentile_indices.argtypes = [C.c_uint64, _u64p, _u64p]
lib.pw_empirical_set_fingerprint_mask.restype = None
lib.pw_empirical_set_fingerprint_mask.argtypes = [C.c_uint64]
lib.pw_empirical_last_stats.restype = None
lib.pw_empirical_last_stats.argtypes = [_u64p]


class EmpiricalError(stage.StageError):
    """a non-zero status of pw_empirical_detect: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_empirical_detect", STATUS

    def decode(self) -> str:
        if self.status == 3:
            return "head at " + stage.describe(4, self.info)
        return f"pc {self.info:#x}" if self.status == 5 else super().decode()


def _partition_map(classes) -> dict:
    return {tuple(cell): k for k, cls in enumerate(classes) for cell in cls}


def _canonical(classes) -> list:
    return sorted(sorted((int(i), int(c)) for i, c in cls) for cls in classes if len(cls) >= 2)


def intersect_partitions(a, b) -> list:
    """cells together in both partitions stay together; a cell missing on either side is a singleton (and is dropped)"""
    ma, mb = _partition_map(a), _partition_map(b)
    groups = {}
    for cell, ka in ma.items():
        if cell in mb:
            groups.setdefault((ka, mb[cell]), []).append(cell)
    return _canonical(groups.values())


@dataclass
class EmpiricalConstraints:
    column_ranges_by_pc: dict = field(default_factory=dict)           # pc -> [(lo, hi)] per column
    equivalence_classes_by_block: dict = field(default_factory=dict)  # start pc -> [[(instruction_idx, column_idx)]]
    pc_counts: dict = field(default_factory=dict)                     # pc -> executions
    debug_info: dict = field(default_factory=lambda: {"air_id_by_pc": {}, "column_names_by_air_id": {}})

    def combine_with(self, other: "EmpiricalConstraints") -> "EmpiricalConstraints":
        """the most conservative combination of two batches, in place (the reference's `combine_with`): ranges min / max column by
        column, partitions intersected, counts added, debug maps merged — which must agree where both have a key"""
        for name in ("air_id_by_pc", "column_names_by_air_id"):
            mine, theirs = self.debug_info[name], other.debug_info[name]
            for k, v in theirs.items():
                if k in mine and mine[k] != v:
                    raise ValueError(f"debug_info.{name}[{k}] differs: {mine[k]!r} and {v!r}")
        for pc, ranges in other.column_ranges_by_pc.items():
            if pc in self.column_ranges_by_pc:
                mine = self.column_ranges_by_pc[pc]
                for i, (lo, hi) in enumerate(ranges[:len(mine)]):
                    mine[i] = (min(mine[i][0], lo), max(mine[i][1], hi))
            else:
                self.column_ranges_by_pc[pc] = [tuple(r) for r in ranges]
        for block, classes in other.equivalence_classes_by_block.items():
            if block in self.equivalence_classes_by_block:
                self.equivalence_classes_by_block[block] = intersect_partitions(self.equivalence_classes_by_block[block], classes)
            else:
                self.equivalence_classes_by_block[block] = _canonical(classes)
        for name in ("air_id_by_pc", "column_names_by_air_id"):
            self.debug_info[name].update(other.debug_info[name])
        for pc, n in other.pc_counts.items():
            self.pc_counts[pc] = self.pc_counts.get(pc, 0) + n
        return self

    def apply_pc_threshold(self, threshold: int = 100) -> "EmpiricalConstraints":
        """a copy without the ranges of pcs, and the classes of blocks, executed fewer than `threshold` times (a block counts as its
        first instruction); counts and debug info are kept"""
        seen = lambda pc: self.pc_counts.get(pc, 0) >= threshold
        return EmpiricalConstraints({pc: list(r) for pc, r in self.column_ranges_by_pc.items() if seen(pc)},
                                    {b: [list(c) for c in cl] for b, cl in self.equivalence_classes_by_block.items() if seen(b)},
                                    dict(self.pc_counts), {k: dict(v) for k, v in self.debug_info.items()})

    def to_json(self) -> str:
        """the text serde_json::to_string_pretty gives the reference's struct: integer keys as decimal strings, ascending"""
        order = lambda d: sorted(d.items())
        doc = {
            "column_ranges_by_pc": {str(pc): [[int(lo), int(hi)] for lo, hi in r] for pc, r in order(self.column_ranges_by_pc)},
            "equivalence_classes_by_block": {str(b): [[{"instruction_idx": int(i), "column_idx": int(c)} for i, c in cls] for cls in cl]
                                             for b, cl in order(self.equivalence_classes_by_block)},
            "debug_info": {"air_id_by_pc": {str(pc): int(a) for pc, a in order(self.debug_info["air_id_by_pc"])},
                           "column_names_by_air_id": {str(a): list(n) for a, n in order(self.debug_info["column_names_by_air_id"])}},
            "pc_counts": {str(pc): int(n) for pc, n in order(self.pc_counts)},
        }
        return json.dumps(doc, indent=2)

    @classmethod
    def from_json(cls, text: str) -> "EmpiricalConstraints":
        doc = json.loads(text)
        dbg = doc.get("debug_info", {})
        return cls({int(pc): [(int(lo), int(hi)) for lo, hi in r] for pc, r in doc["column_ranges_by_pc"].items()},
                   {int(b): [[(int(e["instruction_idx"]), int(e["column_idx"])) for e in c] for c in cl] for b, cl in doc["equivalence_classes_by_block"].items()},
                   {int(pc): int(n) for pc, n in doc["pc_counts"].items()},
                   {"air_id_by_pc": {int(pc): int(a) for pc, a in dbg.get("air_id_by_pc", {}).items()},
                    "column_names_by_air_id": {int(a): list(n) for a, n in dbg.get("column_names_by_air_id", {}).items()}})


def percentile_indices(n: int):
    """pw_empirical_percentile_indices: the positions (n // 100, n * 99 // 100) of the two percentile elements among n sorted values"""
    lo, hi = C.c_uint64(), C.c_uint64()
    lib.pw_empirical_percentile_indices(int(n), C.byref(lo), C.byref(hi))
    return int(lo.value), int(hi.value)


def set_fingerprint_mask(mask: int) -> None:
    """a test hook: ANDed onto both fingerprint halves of this thread's later detect calls; 0 restores the full width"""
    lib.pw_empirical_set_fingerprint_mask(int(mask))


def last_stats() -> dict:
    out = (C.c_uint64 * 6)()
    lib.pw_empirical_last_stats(out)
    return dict(zip(("panels", "seeds", "active_rows", "cells_verified", "peak_bytes", "scratch_bytes"), (int(x) for x in out)))


def detect(airs, blocks, segments=None, bus: int = BUS_EXEC, pc_step: int = 4, scratch_bytes: int = 0, column_names=None) -> EmpiricalConstraints:
    """airs: [(Prover, device trace pointer, log_height)] as for check_segment_buses; blocks: [(start_pc, n_instructions)], ascending
    and non-overlapping; segments: one segment number per AIR entry (None: all 0); column_names: {AIR index: [names]} for the debug
    info. A non-zero status raises EmpiricalError."""
    recs, numbers = stage.air_records(airs, segments)
    blk = (PwBasicBlock * max(len(blocks), 1))()
    for i, (start, count) in enumerate(blocks):
        blk[i] = PwBasicBlock(int(start), int(count))
    handle = stage.call(lib.pw_empirical_detect, "pw_empirical_detect", recs, numbers, len(airs), int(bus), int(pc_step), blk, len(blocks), int(scratch_bytes),
                        error=EmpiricalError)
    try:
        sizes = (C.c_uint64 * 5)()
        lib.pw_empirical_sizes(handle, sizes)
        n_pcs, n_ranges, n_blocks, n_classes, n_cells = (int(x) for x in sizes)
        pcs, counts, air_of = np.zeros(n_pcs, np.uint32), np.zeros(n_pcs, np.uint64), np.zeros(n_pcs, np.uint32)
        roff, ranges = np.zeros(n_pcs + 1, np.uint64), np.zeros((n_ranges, 2), np.uint32)
        starts, coff, eoff = np.zeros(n_blocks, np.uint32), np.zeros(n_blocks + 1, np.uint64), np.zeros(n_classes + 1, np.uint64)
        cells = np.zeros((n_cells, 2), np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        lib.pw_empirical_read_pcs(handle, ptr(pcs), ptr(counts), ptr(air_of), ptr(roff))
        lib.pw_empirical_read_ranges(handle, ptr(ranges))
        lib.pw_empirical_read_blocks(handle, ptr(starts), ptr(coff), ptr(eoff))
        lib.pw_empirical_read_cells(handle, ptr(cells))
    finally:
        lib.pw_empirical_destroy(handle)
    roff, coff, eoff = roff.astype(np.int64), coff.astype(np.int64), eoff.astype(np.int64)
    ranges, cells = ranges.tolist(), cells.tolist()
    out = EmpiricalConstraints()
    for k, pc in enumerate(pcs.tolist()):
        out.column_ranges_by_pc[pc] = [tuple(r) for r in ranges[roff[k]:roff[k + 1]]]
        out.pc_counts[pc] = int(counts[k])
        out.debug_info["air_id_by_pc"][pc] = int(air_of[k])
    for k, start in enumerate(starts.tolist()):
        out.equivalence_classes_by_block[start] = [[tuple(c) for c in cells[eoff[j]:eoff[j + 1]]] for j in range(coff[k], coff[k + 1])]
    used = set(out.debug_info["air_id_by_pc"].values())
    out.debug_info["column_names_by_air_id"] = {int(a): list(names) for a, names in (column_names or {}).items() if int(a) in used}
    return out
