"""Applying APC calls (include/powdr_prover.h `pw_apc_sources_from_traces`, `pw_trace_gather_rows`): from a segment's
instruction-AIR traces on the device and the calls `apc_calls.select_calls` chose, per (APC, AIR) the call-major source matrix the APC
trace generator reads (`OriginalAir`, `Subst` of include/powdr_gpu.h) and per AIR the residual trace — the rows no call covers, which
the original chip still has to prove. Nothing leaves the device.

Direct mode (`pw_apc_sources_from_traces_flags` with `PW_APC_SOURCES_DIRECT`, `pw_apc_sources_tracegen`): `apply_calls(...,
direct=True)` builds no source matrices — the handle keeps the index lists and `ApcSources.apc_traces` writes the APC traces straight
from the chips' traces, which must stay alive and unchanged until the last `apc_traces` call."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import abi, prover, stage
from .apc_calls import Apc, ApcCall, ApcCalls
from .empirical import BUS_EXEC

lib = abi.lib
STATUS = {0: "applied", **stage.texts(2, 4, 7, 11), 12: "two calls of one APC disagree on the AIR of an instruction"}
DIRECT = 1  # PW_APC_SOURCES_DIRECT
TRACEGEN_STATS = ("jobs", "work_items", "tiles_16_byte_loads", "tiles_4_byte_loads", "bytes_written", "scratch_bytes")
STATS = ("covered", "source_bytes", "residual_bytes", "gather_jobs", "tiles_16_byte_loads", "tiles_4_byte_loads", "peak_bytes", "scratch_bytes")

Layout = namedtuple("Layout", "n_calls instructions")  # instructions: [(air, occ)], empty for an APC without calls
Source = namedtuple("Source", "ptr width height rbs")
Residual = namedtuple("Residual", "ptr rows log_height")
GatherJob = namedtuple("GatherJob", "src h_in width idx out h_out")  # src, idx, out: device pointers


class PwGatherJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("h_in", C.c_uint64), ("width", C.c_uint64), ("idx", C.c_void_p), ("out", C.c_void_p), ("h_out", C.c_uint64)]


assert C.sizeof(PwGatherJob) == 48


class PwApcCell(C.Structure):
    _fields_ = [("instr", C.c_uint32), ("col", C.c_uint32), ("apc_col", C.c_uint32)]


class PwApcTraceJob(C.Structure):
    _fields_ = [("apc", C.c_uint32), ("cells", C.POINTER(PwApcCell)), ("n_cells", C.c_size_t), ("d_out", C.c_void_p), ("out_height", C.c_uint64),
                ("out_width", C.c_uint32)]


assert C.sizeof(PwApcCell) == 12 and C.sizeof(PwApcTraceJob) == 48

_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
lib.pw_trace_gather_rows.restype = C.c_int
lib.pw_trace_gather_rows.argtypes = [C.POINTER(PwGatherJob), C.c_size_t]
lib.pw_apc_sources_from_traces.restype = C.c_int
lib.pw_apc_sources_from_traces.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32, _u32p, C.c_size_t, _u32p, _u64p, _u64p, C.c_size_t, C.c_uint32,
                                           C.c_size_t, C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_apc_sources_from_traces_flags.restype = C.c_int
lib.pw_apc_sources_from_traces_flags.argtypes = lib.pw_apc_sources_from_traces.argtypes[:12] + [C.c_uint32] + lib.pw_apc_sources_from_traces.argtypes[12:]
lib.pw_apc_sources_index_bytes.restype = C.c_uint64
lib.pw_apc_sources_index_bytes.argtypes = [C.c_void_p]
lib.pw_apc_sources_tracegen.restype = C.c_int
lib.pw_apc_sources_tracegen.argtypes = [C.c_void_p, C.POINTER(PwApcTraceJob), C.c_size_t]
lib.pw_apc_sources_tracegen_last_stats.restype = None
lib.pw_apc_sources_tracegen_last_stats.argtypes = [_u64p]
lib.pw_apc_sources_destroy.restype = None
lib.pw_apc_sources_destroy.argtypes = [C.c_void_p]
lib.pw_apc_sources_sizes.restype = None
lib.pw_apc_sources_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_apc_sources_layout.restype = C.c_int64
lib.pw_apc_sources_layout.argtypes = [C.c_void_p, C.c_uint32, _u64p, C.c_void_p, C.c_void_p]
lib.pw_apc_sources_source.restype = C.c_int
lib.pw_apc_sources_source.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), _u32p, _u64p, _u32p]
lib.pw_apc_sources_residual.restype = C.c_int
lib.pw_apc_sources_residual.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), _u64p, _u32p]
lib.pw_apc_sources_read_source.restype = C.c_int
lib.pw_apc_sources_read_source.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
lib.pw_apc_sources_read_residual.restype = C.c_int
lib.pw_apc_sources_read_residual.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p]
lib.pw_apc_sources_last_stats.restype = None
lib.pw_apc_sources_last_stats.argtypes = [_u64p]


class ApcSourcesError(stage.StageError):
    """a non-zero status of pw_apc_sources_from_traces: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_apc_sources", STATUS


def last_stats() -> dict:
    out = (C.c_uint64 * 8)()
    lib.pw_apc_sources_last_stats(out)
    return dict(zip(STATS, (int(x) for x in out)))


def tracegen_last_stats() -> dict:
    """of the calling thread's last `ApcSources.apc_traces` (`pw_apc_sources_tracegen_last_stats`)"""
    out = (C.c_uint64 * 6)()
    lib.pw_apc_sources_tracegen_last_stats(out)
    return dict(zip(TRACEGEN_STATS, (int(x) for x in out)))


def trace_jobs(jobs):
    """[(apc, [(instr, col, apc_col)], out_ptr, out_height, out_width)] -> (the PwApcTraceJob array, what keeps its cell arrays alive)"""
    recs, keep = (PwApcTraceJob * max(len(jobs), 1))(), []
    for k, (apc, cells, out_ptr, out_height, out_width) in enumerate(jobs):
        flat = np.ascontiguousarray(np.asarray(list(cells), dtype=np.uint32).reshape(-1, 3))
        keep.append(flat)
        recs[k] = PwApcTraceJob(int(apc), flat.ctypes.data_as(C.POINTER(PwApcCell)) if len(flat) else None, len(flat), int(out_ptr) if out_ptr else None, int(out_height),
                                int(out_width))
    return recs, keep


def gather_rows(jobs) -> None:
    """jobs: [GatherJob(src, h_in, width, idx, out, h_out)] with device pointers: out[c * h_out + i] = src[c * h_in + idx[i]], an index
    0xFFFFFFFF gives a zero row; every word of every output is written, all jobs in one launch (`pw_trace_gather_rows`)"""
    jobs = [GatherJob(*j) for j in jobs]
    recs = (PwGatherJob * max(len(jobs), 1))(*[PwGatherJob(*(int(x) if x is not None else None for x in j)) for j in jobs])
    stage.check(lib.pw_trace_gather_rows(recs, len(jobs)), "pw_trace_gather_rows")


class ApcSources(stage.Handle):
    """`.layout[a]` Layout(n_calls, [(air, occ)]); `.source(a, air)` Source(ptr, width, height, rbs), height 0 where APC a does not
    use the AIR; `.residual(air)` Residual(ptr, rows, log_height) or None for an AIR that takes no part; `.positions`, `.covered`,
    `.source_bytes`, `.residual_bytes`. The device pointers are valid until close(). `.direct`: made by `apply_calls(direct=True)` — no
    source matrix exists (`source()` has height 0 everywhere), `.index_bytes` are the handle's index lists and `apc_traces` writes the
    APC traces from the chips' traces."""

    def __init__(self, handle, widths, direct=False):
        super().__init__(handle, lib.pw_apc_sources_destroy)
        self._widths, self.direct = [int(w) for w in widths], bool(direct)
        self.index_bytes = int(lib.pw_apc_sources_index_bytes(handle))
        sizes = (C.c_uint64 * 6)()
        lib.pw_apc_sources_sizes(handle, sizes)
        self.n_apcs, self.n_airs, self.positions, self.covered, self.source_bytes, self.residual_bytes = (int(x) for x in sizes)
        self.layout = []
        for a in range(self.n_apcs):
            n = C.c_uint64()
            length = lib.pw_apc_sources_layout(handle, a, C.byref(n), None, None)
            air, occ = np.zeros(max(length, 1), np.uint32), np.zeros(max(length, 1), np.uint32)
            if length > 0:
                lib.pw_apc_sources_layout(handle, a, None, air.ctypes.data_as(C.c_void_p), occ.ctypes.data_as(C.c_void_p))
            self.layout.append(Layout(int(n.value), list(zip(air[:length].tolist(), occ[:length].tolist()))))

    def source(self, apc: int, air: int):
        p, w, h, b = C.c_void_p(), C.c_uint32(), C.c_uint64(), C.c_uint32()
        if lib.pw_apc_sources_source(self._h, int(apc), int(air), C.byref(p), C.byref(w), C.byref(h), C.byref(b)) != 0:
            raise IndexError(f"no APC {apc} or no AIR {air}")
        return Source(p.value, int(w.value), int(h.value), int(b.value))

    def residual(self, air: int):
        p, rows, lh = C.c_void_p(), C.c_uint64(), C.c_uint32()
        rc = lib.pw_apc_sources_residual(self._h, int(air), C.byref(p), C.byref(rows), C.byref(lh))
        if rc < 0:
            raise IndexError(f"no AIR {air}")
        return Residual(p.value, int(rows.value), int(lh.value)) if rc else None

    def read_source(self, apc: int, air: int) -> np.ndarray:
        """the source matrix copied to the host: u32[width, height], the words as they lie (Montgomery)"""
        s = self.source(apc, air)
        out = np.zeros((s.width, s.height), np.uint32)
        if out.size:
            abi.check(lib.pw_apc_sources_read_source(self._h, int(apc), int(air), out.ctypes.data_as(C.c_void_p)), "pw_apc_sources_read_source")
        return out

    def read_residual(self, air: int) -> np.ndarray:
        """the residual matrix copied to the host: u32[width, 2^log_height], or None for an AIR that takes no part"""
        r = self.residual(air)
        if r is None:
            return None
        out = np.zeros((self._widths[air], 1 << r.log_height), np.uint32)
        abi.check(lib.pw_apc_sources_read_residual(self._h, int(air), out.ctypes.data_as(C.c_void_p)), "pw_apc_sources_read_residual")
        return out

    def source_airs(self, apc: int) -> list:
        """the AIRs APC apc uses, ascending: entry i of `original_airs(apc)` is AIR source_airs(apc)[i]"""
        return sorted({air for air, _ in self.layout[apc].instructions})

    def original_airs(self, apc: int):
        """the `OriginalAir` array of APC apc (device pointers inside), one entry per AIR of `source_airs(apc)`: what
        `powdr_apc_tracegen_host_tables` takes as h_original_airs"""
        self._needs_matrices("original_airs")
        used = self.source_airs(apc)
        recs = (abi.OriginalAir * max(len(used), 1))()
        for i, air in enumerate(used):
            s = self.source(apc, air)
            recs[i] = abi.OriginalAir(s.width, s.height, s.ptr, s.rbs)
        return recs

    def substs(self, apc: int, cells) -> np.ndarray:
        """cells: [(instr_idx, col, apc_col)] -> the `Subst` rows int32 [n, 4] = {air_index into original_airs(apc), col, row = occ, apc_col}"""
        self._needs_matrices("substs")
        index = {air: i for i, air in enumerate(self.source_airs(apc))}
        ins = self.layout[apc].instructions
        return np.array([(index[ins[k][0]], col, ins[k][1], apc_col) for k, col, apc_col in cells], np.int32).reshape(-1, 4)

    def _needs_matrices(self, what):
        if self.direct:
            raise ValueError(f"{what}: a direct handle has no source matrices; use apc_traces")

    def apc_traces(self, jobs) -> None:
        """jobs: [(apc, [(instr, col, apc_col)], out_ptr, out_height, out_width)], out_ptr a column-major out_width x out_height device
        matrix: out[apc_col * out_height + r] = the cell (instr, col) of call r of the APC, 0 for r >= its calls; columns no cell names
        are not touched. All jobs in one launch (`pw_apc_sources_tracegen`); a direct handle only."""
        recs, keep = trace_jobs(list(jobs))
        stage.check(lib.pw_apc_sources_tracegen(self._h, recs, len(keep)), "pw_apc_sources_tracegen", "" if self.direct else " (the handle is not direct)")

    def residual_segment(self, seg) -> list:
        """seg with the AIRs that took part replaced by their residuals: the AIR list `prove_segment` and `check_segment_buses` take"""
        assert len(seg) == self.n_airs
        out = []
        for air, (pr, ptr, lh) in enumerate(seg):
            r = self.residual(air)
            out.append((pr, ptr, lh) if r is None else (pr, r.ptr, r.log_height))
        return out


def apply_calls(seg, calls, apcs, segments=None, bus: int = BUS_EXEC, min_log_height: int = 0, scratch_bytes: int = 0, direct: bool = False) -> ApcSources:
    """seg: the AIR list [(Prover, device trace pointer, log_height)] `select_calls` took; calls: its `ApcCalls`, or a list of
    ApcCall(apc_id, start, end) ascending in start; apcs: [Apc] or the cycle counts, apc_id = the index; segments: one segment number
    for all AIRs. direct: keep the index lists instead of source matrices (`ApcSources.apc_traces`); the traces of seg must then stay
    alive and unchanged while the handle is used. A non-zero status raises ApcSourcesError."""
    if isinstance(calls, ApcCalls):
        calls = calls.calls
    calls = [ApcCall(*c) for c in calls]
    cycles = [int(a.cycle_count if isinstance(a, Apc) else a[1] if isinstance(a, (tuple, list)) else a) for a in apcs]
    recs, numbers = stage.air_records(seg, segments)
    n, m = len(calls), len(cycles)
    t_cycles = (C.c_uint32 * max(m, 1))(*cycles)
    t_ids = (C.c_uint32 * max(n, 1))(*[int(c.apc_id) for c in calls])
    t_from = (C.c_uint64 * max(n, 1))(*[int(c.start) for c in calls])
    t_to = (C.c_uint64 * max(n, 1))(*[int(c.end) for c in calls])
    head = (recs, numbers, len(seg), int(bus), t_cycles, m, t_ids, t_from, t_to, n, int(min_log_height), int(scratch_bytes))
    fn, args = (lib.pw_apc_sources_from_traces_flags, (*head, DIRECT)) if direct else (lib.pw_apc_sources_from_traces, head)
    return ApcSources(stage.call(fn, "pw_apc_sources_from_traces", *args, error=ApcSourcesError), [pr.width for pr, _, _ in seg], direct=direct)
