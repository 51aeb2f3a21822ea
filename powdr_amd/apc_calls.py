"""Selecting APC calls (include/powdr_prover.h `pw_apc_calls_from_states` / `_from_traces`): what the reference's
`ApcCandidates` (autoprecompiles/src/execution/candidates.rs) decides while an execution runs — which stretches become calls of which
APC, under optimistic constraints checked state by state and with overlapping candidates resolved pair by pair — found on the device
from the whole execution at once. `OptimisticConstraints` is the reference's grouping by step with serde's JSON layout;
`superblock_pc_constraints` the constraints a superblock's start pcs give."""
from __future__ import annotations

import ctypes as C
import json
from collections import namedtuple

import numpy as np

from . import abi, prover, stage
from .empirical import BUS_EXEC

lib = abi.lib
STATUS = {0: "selected", **stage.texts(2, 4, 7, 8, 9, 10)}
COUNTERS = ("matches", "refused", "failed", "aborted", "done", "discarded", "calls")
KIND_NUMBER, KIND_PC, KIND_REGISTER_LIMB = 0, 1, 2

Number = namedtuple("Number", "value")
Pc = namedtuple("Pc", "instr_idx")
RegisterLimb = namedtuple("RegisterLimb", "instr_idx reg limb")
Constraint = namedtuple("Constraint", "left right")
Apc = namedtuple("Apc", "start_pc cycle_count priority constraints", defaults=((),))
ApcCall = namedtuple("ApcCall", "apc_id start end")


class PwApcOperand(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("instr_idx", C.c_uint32), ("reg", C.c_uint32), ("limb", C.c_uint32), ("value", C.c_uint64)]


class PwApcConstraint(C.Structure):
    _fields_ = [("left", PwApcOperand), ("right", PwApcOperand)]


class PwApc(C.Structure):
    _fields_ = [("start_pc", C.c_uint32), ("cycle_count", C.c_uint32), ("priority", C.c_uint64), ("first_constraint", C.c_uint64),
                ("n_constraints", C.c_uint64)]


assert C.sizeof(PwApcOperand) == 24 and C.sizeof(PwApcConstraint) == 48 and C.sizeof(PwApc) == 32

_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_tail = [C.POINTER(PwApc), C.c_size_t, C.POINTER(PwApcConstraint), C.c_size_t, C.c_size_t, C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_apc_calls_from_states.restype = C.c_int
lib.pw_apc_calls_from_states.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32] + _tail
lib.pw_apc_calls_from_traces.restype = C.c_int
lib.pw_apc_calls_from_traces.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32, C.c_uint32] + _tail
lib.pw_apc_calls_from_traces_registers.restype = C.c_int
lib.pw_apc_calls_from_traces_registers.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t] + [C.c_uint32] * 7 + [_u32p] + _tail
lib.pw_apc_calls_destroy.restype = None
lib.pw_apc_calls_destroy.argtypes = [C.c_void_p]
lib.pw_apc_calls_sizes.restype = None
lib.pw_apc_calls_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_apc_calls_read_calls.restype = None
lib.pw_apc_calls_read_calls.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_apc_calls_read_counters.restype = None
lib.pw_apc_calls_read_counters.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_apc_calls_read_time_keys.restype = None
lib.pw_apc_calls_read_time_keys.argtypes = [C.c_void_p, C.c_void_p]
lib.pw_apc_calls_set_long_threshold.restype = None
lib.pw_apc_calls_set_long_threshold.argtypes = [C.c_uint64]
lib.pw_apc_calls_last_stats.restype = None
lib.pw_apc_calls_last_stats.argtypes = [_u64p]


# ---- optimistic constraints -------------------------------------------------------------------------------------------------------
def _literals(c: Constraint) -> list:
    """the constraint's distinct literals, left before right (the reference's `unique_references`)"""
    out = []
    for e in (c.left, c.right):
        if not isinstance(e, Number) and e not in out:
            out.append(e)
    return out


def step_of(c: Constraint) -> int:
    """the first step at which the constraint can be checked: the largest instr_idx among its literals, 0 without one"""
    return max((l.instr_idx for l in _literals(c)), default=0)


def _expr_json(e):
    if isinstance(e, Number):
        return {"Number": int(e.value)}
    val = "Pc" if isinstance(e, Pc) else {"RegisterLimb": [int(e.reg), int(e.limb)]}
    return {"Literal": {"instr_idx": int(e.instr_idx), "val": val}}


def _expr_from_json(j):
    if "Number" in j:
        return Number(int(j["Number"]))
    lit = j["Literal"]
    if lit["val"] == "Pc":
        return Pc(int(lit["instr_idx"]))
    reg, limb = lit["val"]["RegisterLimb"]
    return RegisterLimb(int(lit["instr_idx"]), int(reg), int(limb))


class OptimisticConstraints:
    """`fetches_by_step` {step: [("Pc",) | ("Register", reg)]}: what a later constraint reads of this step's state, in the order the
    constraints name it (not deduplicated, as in the reference); `constraints_to_check_by_step` {step: [Constraint]}."""

    def __init__(self, fetches_by_step=None, constraints_to_check_by_step=None):
        self.fetches_by_step = dict(fetches_by_step or {})
        self.constraints_to_check_by_step = dict(constraints_to_check_by_step or {})

    @classmethod
    def from_constraints(cls, constraints) -> "OptimisticConstraints":
        fetches, checks = {}, {}
        data = [(step_of(c), _literals(c), c) for c in (Constraint(*c) for c in constraints)]
        for step, lits, _ in data:
            for l in lits:
                if step > l.instr_idx:
                    fetches.setdefault(l.instr_idx, []).append(("Pc",) if isinstance(l, Pc) else ("Register", l.reg))
        for step, _, c in data:
            checks.setdefault(step, []).append(c)
        return cls(dict(sorted(fetches.items())), dict(sorted(checks.items())))

    def constraints(self) -> list:
        """all constraints, by step"""
        return [c for _, cs in sorted(self.constraints_to_check_by_step.items()) for c in cs]

    def to_json(self) -> dict:
        """serde's layout: integer keys as decimal strings, externally tagged enums"""
        return {"fetches_by_step": {str(k): ["Pc" if f == ("Pc",) else {"Register": int(f[1])} for f in v] for k, v in self.fetches_by_step.items()},
                "constraints_to_check_by_step": {str(k): [{"left": _expr_json(c.left), "right": _expr_json(c.right)} for c in v]
                                                 for k, v in self.constraints_to_check_by_step.items()}}

    def dumps(self) -> str:
        return json.dumps(self.to_json())

    @classmethod
    def from_json(cls, j) -> "OptimisticConstraints":
        if isinstance(j, str):
            j = json.loads(j)
        fetches = {int(k): [("Pc",) if f == "Pc" else ("Register", int(f["Register"])) for f in v] for k, v in j["fetches_by_step"].items()}
        checks = {int(k): [Constraint(_expr_from_json(c["left"]), _expr_from_json(c["right"])) for c in v]
                  for k, v in j["constraints_to_check_by_step"].items()}
        return cls(dict(sorted(fetches.items())), dict(sorted(checks.items())))

    def __eq__(self, other):
        return (isinstance(other, OptimisticConstraints) and self.fetches_by_step == other.fetches_by_step
                and self.constraints_to_check_by_step == other.constraints_to_check_by_step)


def superblock_pc_constraints(start_pcs_by_instruction) -> list:
    """[(instr_idx, start pc)] of a superblock's basic blocks (the reference's `instruction_indexed_start_pcs`) -> the constraints
    `pc of state instr_idx == start pc`, one per block"""
    return [Constraint(Pc(int(i)), Number(int(pc))) for i, pc in start_pcs_by_instruction]


def instruction_indexed_start_pcs(blocks) -> list:
    """[(start_pc, n_instructions)] of a superblock's blocks in order -> [(index of the block's first instruction, start_pc)]"""
    out, idx = [], 0
    for start, n in blocks:
        out.append((idx, int(start)))
        idx += int(n)
    return out


# ---- the C call ---------------------------------------------------------------------------------------------------------------------
class ApcCallsError(stage.StageError):
    """a non-zero status of pw_apc_calls_from_*: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_apc_calls", STATUS


def set_long_threshold(n: int) -> None:
    """a test hook: components of more than n candidates take the long path in this thread's later calls; 0 restores the default"""
    lib.pw_apc_calls_set_long_threshold(int(n))


def last_stats() -> dict:
    out = (C.c_uint64 * 7)()
    lib.pw_apc_calls_last_stats(out)
    return dict(zip(("candidates", "valid", "components", "longest_component", "long_components", "peak_bytes", "scratch_bytes"), (int(x) for x in out)))


def _operand(e) -> PwApcOperand:
    if isinstance(e, Number):
        return PwApcOperand(KIND_NUMBER, 0, 0, 0, int(e.value))
    if isinstance(e, Pc):
        return PwApcOperand(KIND_PC, int(e.instr_idx), 0, 0, 0)
    if isinstance(e, RegisterLimb):
        return PwApcOperand(KIND_REGISTER_LIMB, int(e.instr_idx), int(e.reg), int(e.limb), 0)
    raise ValueError(f"no operand: {e!r}")


def tables(apcs):
    """[Apc] (constraints: a list of Constraint or an OptimisticConstraints) -> the two host arrays of the C call and their lengths"""
    flat, rows = [], []
    for a in apcs:
        a = Apc(*a)
        cs = a.constraints.constraints() if isinstance(a.constraints, OptimisticConstraints) else [Constraint(*c) for c in a.constraints]
        rows.append((int(a.start_pc), int(a.cycle_count), int(a.priority), len(flat), len(cs)))
        flat += cs
    t_apcs = (PwApc * max(len(rows), 1))(*[PwApc(*r) for r in rows])
    t_cons = (PwApcConstraint * max(len(flat), 1))(*[PwApcConstraint(_operand(c.left), _operand(c.right)) for c in flat])
    return t_apcs, len(rows), t_cons, len(flat)


class ApcCalls(stage.Handle):
    """`.calls` [ApcCall(apc_id, start, end)] in insertion order; `.counters` per APC {matches, refused, failed, aborted, done,
    discarded, calls}; `.covered` the positions inside calls; `.time_keys` (trace route) the time key of every position."""

    def __init__(self, handle):
        super().__init__(handle, lib.pw_apc_calls_destroy)
        sizes = (C.c_uint64 * 5)()
        lib.pw_apc_calls_sizes(handle, sizes)
        n_calls, n_apcs, self.covered, self.n_states, n_keys = (int(x) for x in sizes)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        ids, start, end = np.zeros(n_calls, np.uint32), np.zeros(n_calls, np.uint64), np.zeros(n_calls, np.uint64)
        lib.pw_apc_calls_read_calls(handle, ptr(ids), ptr(start), ptr(end))
        self.calls = [ApcCall(a, s, e) for a, s, e in zip(ids.tolist(), start.tolist(), end.tolist())]
        cnt = np.zeros((n_apcs, len(COUNTERS)), np.uint64)
        lib.pw_apc_calls_read_counters(handle, ptr(cnt))
        self.counters = [dict(zip(COUNTERS, row)) for row in cnt.tolist()]
        keys = np.zeros(n_keys, np.uint64)
        lib.pw_apc_calls_read_time_keys(handle, ptr(keys))
        self.time_keys = keys.tolist()


def select_calls(states_or_segment, apcs, regs=None, limb_bits: int = 8, final_pc=None, segments=None, bus: int = BUS_EXEC,
                 scratch_bytes: int = 0, registers=None) -> ApcCalls:
    """states_or_segment: the pcs of the execution's N + 1 states in order (a CUDA int32 / uint32 tensor read in place, or anything
    numpy turns into 32-bit words) with `regs` the register values, one row of N + 1 values per register (column-major on the device)
    — or the AIR list [(Prover, device trace pointer, log_height)] of `execution_blocks.detect` with `final_pc`, the pc after the last
    row, and `segments` naming one segment. On that route `registers` = dict(n_regs=32, initial=None, reg_as=1, ptr_step=4, memory_bus=1)
    (every key optional) reads the registers the constraints name off the memory bus (§5s): n_regs bounds a literal's register, initial
    is None or n_regs words, the machine at the segment's start; without it a register literal is refused as before.
    apcs: [Apc(start_pc, cycle_count, priority, constraints)], apc_id = the index.
    A non-zero status raises ApcCallsError."""
    t_apcs, n_apcs, t_cons, n_cons = tables(apcs)
    tail = (t_apcs, n_apcs, t_cons, n_cons, int(scratch_bytes))
    if stage.is_air_list(states_or_segment):
        if final_pc is None or regs is not None:
            raise ValueError("the trace route: final_pc, and no registers")
        recs, numbers = stage.air_records(states_or_segment, segments)
        head = (recs, numbers, len(states_or_segment), int(bus))
        if registers is None:
            fn, what, args = lib.pw_apc_calls_from_traces, "pw_apc_calls_from_traces", (*head, int(final_pc))
        else:
            unknown = set(registers) - {"n_regs", "initial", "reg_as", "ptr_step", "memory_bus"}
            if unknown:
                raise ValueError(f"registers: unknown keys {sorted(unknown)}")
            n_regs, initial = int(registers.get("n_regs", 32)), registers.get("initial")
            if initial is not None and len(initial) != n_regs:
                raise ValueError("registers: initial holds one word per register")
            t_init = None if initial is None else (C.c_uint32 * max(n_regs, 1))(*[int(w) for w in initial])
            fn, what = lib.pw_apc_calls_from_traces_registers, "pw_apc_calls_from_traces_registers"
            args = (*head, int(registers.get("memory_bus", 1)), int(final_pc), int(registers.get("reg_as", 1)), int(registers.get("ptr_step", 4)), n_regs, int(limb_bits),
                    t_init)
    else:
        import torch

        if registers is not None:
            raise ValueError("registers: on the trace route only")
        keep_pcs, n_states = stage.device_words(states_or_segment, "the pcs")
        keep_regs, n_regs = None, 0
        if regs is not None:
            if hasattr(regs, "data_ptr"):
                n_regs = regs.numel() // n_states if n_states else 0
            else:
                regs = np.asarray(regs, dtype=np.uint32).reshape(-1, n_states) if n_states else np.zeros((0, 0), np.uint32)
                n_regs = regs.shape[0]
            keep_regs, n_words = stage.device_words(regs, "the registers")
            if n_words != n_regs * n_states:
                raise ValueError("the registers: one row of n_states values per register")
        torch.cuda.synchronize()  # the library reads on its own launch stream
        fn, what = lib.pw_apc_calls_from_states, "pw_apc_calls_from_states"
        args = (keep_pcs.data_ptr() if keep_pcs is not None else None, keep_regs.data_ptr() if keep_regs is not None else None, n_states, n_regs, int(limb_bits))
    return ApcCalls(stage.call(fn, what, *args, *tail, error=ApcCallsError))
