"""Cutting one execution into segments (include/powdr_prover.h `pw_execution_segments_from_traces`): from the
instruction-AIR traces of one long execution on the device, and optionally the calls `apc_calls.select_calls` chose for it, the greedy
cut under a height cap per class and a cell budget that counts a call as ONE row of its APC and never falls inside a call. The
handle keeps, per (segment, AIR), the list of the AIR's rows in the segment — what `apc_sources.gather_rows` takes — and no matrices:
`ExecutionSegments.segment(s)` gathers a segment into tensors of its own. With calls the original trace of a segment may be taller
than the cap: the cap binds the residuals and the APC traces, which is what gets proven.

With `system=SystemMeter(...)` (`pw_execution_segments_from_traces_metered`) the cut also meters the system AIRs that
`close_segment` gives a segment: the distinct memory blocks it touches (the boundary AIR's rows, B), the tree nodes above them (the
memory Merkle AIR's rows, M) and 2 M, an upper BOUND on the Poseidon2 chip's rows (the chip dedupes by input words, so its true height
depends on the hashes). Each is a limit of the cut and, under max_cells, a term of the cell sum."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import abi, prover, stage
from .apc_calls import Apc, ApcCall, ApcCalls
from .apc_sources import GatherJob, gather_rows
from .empirical import BUS_EXEC
from .execution_states import BUS_MEMORY

lib = abi.lib
STATUS = {0: "cut", **stage.texts(2, 4, 7, 11), 13: "nothing fits under max_cells", 14: "more than max_segments segments",
          15: "a memory-bus tuple that has no key"}
STATS = ("segments", "classes", "cell_probes", "snapped_cuts", "peak_bytes", "scratch_bytes")
METER_STATS = ("accesses", "tiles", "table_peak_slots", "nodes_past_the_cuts", "synchronisations", "tables")
BOUNDARY_WIDTH, MERKLE_WIDTH, POSEIDON2_WIDTH = 18, 55, 307  # system_airs.BOUNDARY_WIDTH, memory_tree.MERKLE_WIDTH, system_airs.POSEIDON2_WIDTH


class PwSegmentLimits(C.Structure):
    _fields_ = [("max_log_height", C.c_uint32), ("min_log_height", C.c_uint32), ("max_cells", C.c_uint64), ("max_segments", C.c_uint64)]


assert C.sizeof(PwSegmentLimits) == 24


class PwSystemMeter(C.Structure):
    _fields_ = [("memory_bus", C.c_uint32), ("tree_height", C.c_uint32), ("max_log_height", C.c_uint32 * 3), ("width", C.c_uint32 * 3)]


assert C.sizeof(PwSystemMeter) == 32


@dataclass(frozen=True)
class SystemMeter:
    """what `cut(system=)` meters: the memory tree's height (1 .. 30), the log2 caps of the boundary AIR, the Merkle AIR and the
    Poseidon2 bound — None: the cut's own max_log_height for all three, an int: that cap for all three, or (b, m, p) — the widths the
    three count with under max_cells (0 leaves a term out) and the memory bus"""
    tree_height: int = 30
    max_log_height: object = None
    widths: tuple = (BOUNDARY_WIDTH, MERKLE_WIDTH, POSEIDON2_WIDTH)
    memory_bus: int = BUS_MEMORY

    def record(self, max_log_height: int) -> PwSystemMeter:
        caps = self.max_log_height
        caps = (max_log_height,) * 3 if caps is None else (caps,) * 3 if isinstance(caps, int) else tuple(caps)
        widths = tuple(self.widths)
        if len(caps) != 3 or len(widths) != 3:
            raise ValueError("SystemMeter: three caps and three widths (boundary, Merkle, Poseidon2)")
        for name, v in (("tree_height", self.tree_height), ("memory_bus", self.memory_bus), *(("max_log_height", c) for c in caps), *(("widths", w) for w in widths)):
            if not 0 <= int(v) < 1 << 32:
                raise ValueError(f"SystemMeter: {name} out of range")
        return PwSystemMeter(int(self.memory_bus), int(self.tree_height), (C.c_uint32 * 3)(*[int(c) for c in caps]), (C.c_uint32 * 3)(*[int(w) for w in widths]))


def padded_sys(n: int, min_log_height: int = 0) -> int:
    """the height a system AIR of n rows is counted with: 0 for none, else at least 2 (no generator returns one row)"""
    return 0 if n == 0 else max(2, 1 << min_log_height, 1 << (int(n) - 1).bit_length())

_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
lib.pw_execution_segments_from_traces.restype = C.c_int
lib.pw_execution_segments_from_traces.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32, C.c_uint32, _u32p, _u32p, C.c_size_t, _u32p, _u64p, _u64p,
                                                  C.c_size_t, C.POINTER(PwSegmentLimits), C.c_size_t, C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_execution_segments_destroy.restype = None
lib.pw_execution_segments_destroy.argtypes = [C.c_void_p]
lib.pw_execution_segments_sizes.restype = None
lib.pw_execution_segments_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_execution_segments_read_bounds.restype = None
lib.pw_execution_segments_read_bounds.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_execution_segments_read_heights.restype = None
lib.pw_execution_segments_read_heights.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_execution_segments_rows.restype = C.c_int
lib.pw_execution_segments_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), _u64p, _u32p]
lib.pw_execution_segments_read_lists.restype = C.c_int
lib.pw_execution_segments_read_lists.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
lib.pw_execution_segments_last_stats.restype = None
lib.pw_execution_segments_last_stats.argtypes = [_u64p]
lib.pw_execution_segments_from_traces_metered.restype = C.c_int
lib.pw_execution_segments_from_traces_metered.argtypes = lib.pw_execution_segments_from_traces.argtypes[:13] + [C.POINTER(PwSystemMeter)] + \
    lib.pw_execution_segments_from_traces.argtypes[13:]
lib.pw_execution_segments_read_system_heights.restype = None
lib.pw_execution_segments_read_system_heights.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_execution_segments_last_meter_stats.restype = None
lib.pw_execution_segments_last_meter_stats.argtypes = [_u64p]
lib.pw_execution_segments_set_meter_tile.restype = None
lib.pw_execution_segments_set_meter_tile.argtypes = [C.c_uint64]


class ExecutionSegmentsError(stage.StageError):
    """a non-zero status of pw_execution_segments_from_traces: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_execution_segments", STATUS

    def decode(self) -> str:
        if self.status == 15:
            return "air %d, interaction %d, row %d" % stage.unpack_witness(self.info)
        return f"position {self.info}" if self.status in (13, 14) else super().decode()


def last_stats() -> dict:
    out = (C.c_uint64 * 6)()
    lib.pw_execution_segments_last_stats(out)
    return dict(zip(STATS, (int(x) for x in out)))


def last_meter_stats() -> dict:
    """of this thread's last metered cut: accesses walked, tiles, the node table's most slots, nodes inserted past the cuts, the host
    synchronisations of the per-segment loop, node tables cleared; zeros after an unmetered cut"""
    out = (C.c_uint64 * 6)()
    lib.pw_execution_segments_last_meter_stats(out)
    return dict(zip(METER_STATS, (int(x) for x in out)))


def set_meter_tile(n: int) -> None:
    """a test knob of this thread: the positions per tile of the meter (0 = the default); results do not depend on it"""
    lib.pw_execution_segments_set_meter_tile(int(n))


class ExecutionSegments(stage.Handle):
    """`.bounds` [b_0 .. b_S]; `.starts` [(pc, time key)] per segment; `.final_pc`; `.first_call` [S + 1]; `.heights[s]` {air or
    ("apc", a): rows} (classes without rows left out); `.calls(s)` the segment's ApcCalls re-based to it; `.rows(s, air)` (device
    pointer of the row list, rows, log_height) or None; `.segment(s)` the segment's traces, gathered. `.n_segments`, `.n_airs`,
    `.n_apcs`, `.positions`, `.covered`, `.list_bytes`. `.system_heights[s]` = (B, M, P) of a metered cut — boundary rows, Merkle rows,
    the bound 2 M on the Poseidon2 chip's rows — and (0, 0, 0) without `system=`. The lists are valid until close()."""

    def __init__(self, handle, seg, calls):
        super().__init__(handle, lib.pw_execution_segments_destroy)
        self._seg, self._calls = list(seg), list(calls)
        sizes = (C.c_uint64 * 6)()
        lib.pw_execution_segments_sizes(handle, sizes)
        self.n_segments, self.n_airs, self.n_apcs, self.positions, self.covered, self.list_bytes = (int(x) for x in sizes)
        S, classes = self.n_segments, self.n_airs + self.n_apcs
        b, keys, pcs, first = np.zeros(S + 1, np.uint64), np.zeros(max(S, 1), np.uint64), np.zeros(S + 1, np.uint32), np.zeros(S + 1, np.uint64)
        lib.pw_execution_segments_read_bounds(handle, *(x.ctypes.data_as(C.c_void_p) for x in (b, keys, pcs, first)))
        rows = np.zeros(max(S * classes, 1), np.uint64)
        lib.pw_execution_segments_read_heights(handle, rows.ctypes.data_as(C.c_void_p))
        self.bounds = [int(x) for x in b]
        self.starts = [(int(pcs[s]), int(keys[s])) for s in range(S)]
        self.final_pc = int(pcs[S])
        self.first_call = [int(x) for x in first]
        sys_rows = np.zeros(max(3 * S, 1), np.uint64)
        lib.pw_execution_segments_read_system_heights(handle, sys_rows.ctypes.data_as(C.c_void_p))
        self.system_heights = [tuple(int(x) for x in sys_rows[3 * s:3 * s + 3]) for s in range(S)]
        self.heights = []
        for s in range(S):
            row = rows[s * classes:(s + 1) * classes]
            self.heights.append({(int(c) if c < self.n_airs else ("apc", int(c) - self.n_airs)): int(row[c]) for c in np.nonzero(row)[0]})

    def calls(self, s: int) -> list:
        """the calls of segment s as positions of the segment: what `apply_calls(self.segment(s), ...)` takes"""
        b = self.bounds[s]
        return [ApcCall(c.apc_id, c.start - b, c.end - b) for c in self._calls[self.first_call[s]:self.first_call[s + 1]]]

    def rows(self, s: int, air: int):
        p, n, lh = C.c_void_p(), C.c_uint64(), C.c_uint32()
        rc = lib.pw_execution_segments_rows(self._h, int(s), int(air), C.byref(p), C.byref(n), C.byref(lh))
        if rc < 0:
            raise IndexError(f"no segment {s} or no AIR {air}")
        return (p.value, int(n.value), int(lh.value)) if rc else None

    def read_lists(self) -> dict:
        """{(segment, air): u32[2^log_height]} — every row list copied to the host in one copy (`pw_execution_segments_read_lists`)"""
        words, base = np.zeros(max(self.list_bytes // 4, 1), np.uint32), C.c_void_p()
        abi.check(lib.pw_execution_segments_read_lists(self._h, words.ctypes.data_as(C.c_void_p), C.byref(base)), "pw_execution_segments_read_lists")
        out = {}
        for s in range(self.n_segments):
            for air in range(self.n_airs):
                r = self.rows(s, air)
                if r is not None:
                    at = (r[0] - base.value) // 4
                    out[(s, air)] = words[at:at + (1 << r[2])]
        return out

    def segment(self, s: int, buffers=None) -> list:
        """[(air index, Prover, tensor i32[width, 2^log_height] column-major on the device, log_height)] for the AIRs with rows in
        segment s: the tensors are allocated here (or taken from buffers {air: a contiguous i32 tensor of width x 2^log_height
        words}) and filled by ONE `gather_rows` call, every word written; AIRs without rows are left out"""
        import torch

        out, jobs = [], []
        for air, (pr, ptr, lh) in enumerate(self._seg):
            r = self.rows(s, air)
            if r is None:
                continue
            if buffers is not None and air in buffers:
                t = buffers[air]
                if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != pr.width << r[2]:
                    raise ValueError(f"segment: the buffer of AIR {air} is no contiguous i32 tensor of {pr.width} x {1 << r[2]} words")
                t = t.view(pr.width, 1 << r[2])
            else:
                t = torch.empty((pr.width, 1 << r[2]), dtype=torch.int32, device="cuda")
            jobs.append(GatherJob(ptr, 1 << lh, pr.width, r[0], t.data_ptr(), 1 << r[2]))
            out.append((air, pr, t, r[2]))
        gather_rows(jobs)
        return out


def cut(seg, max_log_height: int, final_pc: int, calls=None, apcs=None, apc_widths=None, min_log_height: int = 0, max_cells: int = 0, max_segments: int = 0,
        segments=None, bus: int = BUS_EXEC, scratch_bytes: int = 0, system: SystemMeter | None = None) -> ExecutionSegments:
    """seg: the AIR list [(Prover, device trace pointer, log_height)] of ONE execution; calls: the `ApcCalls` of `select_calls` on it, or
    a list of ApcCall(apc_id, start, end) ascending in start; apcs: [Apc] or the cycle counts, apc_id = the index; apc_widths: the
    APC traces' widths (needed under max_cells). A class holds at most 2^max_log_height rows per segment; max_cells (0: no bound)
    bounds the sum of width x padded height, heights padded to at least 2^min_log_height; max_segments 0 = 2^20. system: None (the
    cut as it always was) or a SystemMeter, whose three heights become limits of the cut and terms of the cell sum. A non-zero status
    raises ExecutionSegmentsError."""
    if isinstance(calls, ApcCalls):
        calls = calls.calls
    calls = [ApcCall(*c) for c in (calls or [])]
    apcs = list(apcs or [])
    if calls and not apcs:
        raise ValueError("cut: calls without apcs")
    cycles = [int(a.cycle_count if isinstance(a, Apc) else a[1] if isinstance(a, (tuple, list)) else a) for a in apcs]
    if apc_widths is not None and len(apc_widths) != len(cycles):
        raise ValueError("cut: one width per APC")
    for name, v, top in (("max_log_height", max_log_height, 1 << 32), ("min_log_height", min_log_height, 1 << 32), ("max_cells", max_cells, 1 << 64),
                         ("max_segments", max_segments, 1 << 64), ("final_pc", final_pc, 1 << 32)):
        if not 0 <= int(v) < top:
            raise ValueError(f"cut: {name} out of range")
    recs, numbers = stage.air_records(seg, segments)
    n, m = len(calls), len(cycles)
    t_cycles = (C.c_uint32 * max(m, 1))(*cycles)
    t_widths = (C.c_uint32 * max(m, 1))(*[int(w) for w in apc_widths]) if apc_widths is not None else None
    t_ids = (C.c_uint32 * max(n, 1))(*[int(c.apc_id) for c in calls])
    t_from = (C.c_uint64 * max(n, 1))(*[int(c.start) for c in calls])
    t_to = (C.c_uint64 * max(n, 1))(*[int(c.end) for c in calls])
    limits = PwSegmentLimits(int(max_log_height), int(min_log_height), int(max_cells), int(max_segments))
    if system is None:
        handle = stage.call(lib.pw_execution_segments_from_traces, "pw_execution_segments_from_traces", recs, numbers, len(seg), int(bus), int(final_pc), t_cycles,
                            t_widths, m, t_ids, t_from, t_to, n, C.byref(limits), int(scratch_bytes), error=ExecutionSegmentsError)
    else:
        meter = system.record(int(max_log_height))
        handle = stage.call(lib.pw_execution_segments_from_traces_metered, "pw_execution_segments_from_traces_metered", recs, numbers, len(seg), int(bus), int(final_pc),
                            t_cycles, t_widths, m, t_ids, t_from, t_to, n, C.byref(limits), C.byref(meter), int(scratch_bytes), error=ExecutionSegmentsError)
    return ExecutionSegments(handle, seg, calls)
