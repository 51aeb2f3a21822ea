"""The states of an execution from its traces (include/powdr_prover.h `pw_execution_states_from_traces`): the pcs, the
requested registers and the time keys of one segment's N + 1 states, built on the device from the instruction AIRs' traces — positions
and pcs from the execution bridge as in §5r, registers from the memory bus's sends in time order — and left there in the layout
`pw_apc_calls_from_states` reads. `apc_calls.select_calls(..., registers=...)` uses the same stage without a table that leaves."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, prover, stage
from .empirical import BUS_EXEC

lib = abi.lib
BUS_MEMORY, REGISTER_AS, REGISTER_PTR_STEP = 1, 1, 4
STATUS = {0: "built", **stage.texts(2, 4, 7, 8, 9, 10)}

_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
lib.pw_execution_states_from_traces.restype = C.c_int
lib.pw_execution_states_from_traces.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u32p,
                                                C.c_size_t, _u32p, C.c_size_t, C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_execution_states_destroy.restype = None
lib.pw_execution_states_destroy.argtypes = [C.c_void_p]
lib.pw_execution_states_sizes.restype = None
lib.pw_execution_states_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_execution_states_device.restype = None
lib.pw_execution_states_device.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
lib.pw_execution_states_read.restype = C.c_int
lib.pw_execution_states_read.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_execution_states_last_stats.restype = None
lib.pw_execution_states_last_stats.argtypes = [_u64p]


class ExecutionStatesError(stage.StageError):
    """a non-zero status of pw_execution_states_from_traces: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_execution_states", STATUS


def last_stats() -> dict:
    out = (C.c_uint64 * 5)()
    lib.pw_execution_states_last_stats(out)
    return dict(zip(("sends", "kept", "fill_tile", "peak_bytes", "scratch_bytes"), (int(x) for x in out)))


class ExecutionStates(stage.Handle):
    """`.n_states` = N + 1, `.n_regs`, `.sends` (register sends read), `.bytes` held on the device; `.d_pcs`, `.d_regs`, `.d_time_keys` the
    device pointers (valid until close()); `.pcs()` u32[N + 1], `.regs()` u32[n_regs, N + 1], `.time_keys` [N] copied to the host."""

    def __init__(self, handle):
        super().__init__(handle, lib.pw_execution_states_destroy)
        sizes = (C.c_uint64 * 4)()
        lib.pw_execution_states_sizes(handle, sizes)
        self.n_states, self.n_regs, self.sends, self.bytes = (int(x) for x in sizes)
        p, r, k = C.c_void_p(), C.c_void_p(), C.c_void_p()
        lib.pw_execution_states_device(handle, C.byref(p), C.byref(r), C.byref(k))
        self.d_pcs, self.d_regs, self.d_time_keys = p.value, r.value, k.value
        self._keys = None

    def _read(self, pcs=None, regs=None, keys=None):
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        abi.check(lib.pw_execution_states_read(self._h, ptr(pcs), ptr(regs), ptr(keys)), "pw_execution_states_read")

    def pcs(self) -> np.ndarray:
        out = np.zeros(self.n_states, np.uint32)
        self._read(pcs=out)
        return out

    def regs(self) -> np.ndarray:
        out = np.zeros((self.n_regs, self.n_states), np.uint32)
        if out.size:
            self._read(regs=out)
        return out

    @property
    def time_keys(self) -> list:
        if self._keys is None:
            out = np.zeros(self.n_states - 1, np.uint64)
            if out.size:
                self._read(keys=out)
            self._keys = out.tolist()
        return self._keys


def states_from_traces(seg, regs, final_pc, initial_regs=None, segments=None, bus: int = BUS_EXEC, memory_bus: int = BUS_MEMORY, reg_as: int = REGISTER_AS,
                       ptr_step: int = REGISTER_PTR_STEP, scratch_bytes: int = 0) -> ExecutionStates:
    """seg: the AIR list [(Prover, device trace pointer, log_height)] of `execution_blocks.detect`; regs: distinct register numbers, row
    k of the table is regs[k]; final_pc: the pc after the last row; initial_regs: None or one word per entry of regs, the machine at the
    segment's start; segments: one segment number for all AIRs. A non-zero status raises ExecutionStatesError."""
    regs = [int(r) for r in regs]
    recs, numbers = stage.air_records(seg, segments)
    t_regs = (C.c_uint32 * max(len(regs), 1))(*regs)
    t_init = None
    if initial_regs is not None:
        if len(initial_regs) != len(regs):
            raise ValueError("initial_regs: one word per requested register")
        t_init = (C.c_uint32 * max(len(regs), 1))(*[int(w) for w in initial_regs])
    return ExecutionStates(stage.call(lib.pw_execution_states_from_traces, "pw_execution_states_from_traces", recs, numbers, len(seg), int(bus), int(memory_bus),
                                      int(final_pc), int(reg_as), int(ptr_step), t_regs, len(regs), t_init, int(scratch_bytes), error=ExecutionStatesError))
