"""The Python side of a trace pipeline's entry contract (the C++ side is csrc/trace_entry.hpp): the AIR records every
entry point takes, the handle its result lives in, the one way a C call answers — return code, status, info, handle — and what each
of them becomes in Python. -1 is `Malformed`, another non-zero return code `abi.HipError`, a non-zero status the stage's `StageError`.
Depends on `abi` alone; `empirical`, `execution_blocks`, `apc_calls`, `execution_states`, `apc_sources` and `execution_segments` bind
their entry points through it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi

ROW_BITS, INTERACTION_BITS = 26, 20  # the packed witness (air | interaction | row) of status 8


class PwSegmentAir(C.Structure):
    _fields_ = [("prover", C.c_void_p), ("d_trace", C.c_void_p), ("log_height", C.c_uint32), ("flags", C.c_uint32)]


def air_records(seg, segments=None, flags=None):
    """[(Prover, device trace pointer, log_height)], with `segments` one segment number and with `flags` one flag word per AIR -> the C
    call's AIR records and segment numbers (or None)"""
    n = len(seg)
    recs = (PwSegmentAir * max(n, 1))()
    for i, (pr, ptr, lh) in enumerate(seg):
        recs[i] = PwSegmentAir(pr._h, ptr, lh, flags[i] if flags is not None else 0)
    numbers = None
    if segments is not None:
        assert len(segments) == n
        numbers = (C.c_uint32 * max(n, 1))(*[int(s) for s in segments])
    return recs, numbers


def is_air_list(x) -> bool:
    """an AIR list [(Prover, device trace pointer, log_height)], not a list of words: the trace route of an entry point with two"""
    return isinstance(x, (list, tuple)) and len(x) > 0 and isinstance(x[0], tuple) and hasattr(x[0][0], "_h")


def device_words(x, what):
    """a CUDA int32 / uint32 tensor read in place, or anything numpy turns into 32-bit words copied to the device -> (tensor or None,
    words). The library reads on its own launch stream: the caller synchronises before the C call."""
    import torch

    if hasattr(x, "data_ptr"):
        if not x.is_cuda or x.dtype not in (torch.int32, torch.uint32) or not x.is_contiguous():
            raise ValueError(f"{what} on the device: a contiguous int32 / uint32 tensor")
        return x, x.numel()
    words = np.ascontiguousarray(np.asarray(x, dtype=np.uint32).reshape(-1))
    return (torch.from_numpy(words.view(np.int32)).cuda() if len(words) else None), len(words)


class Handle:
    """owns the handle of a C call's result: destroyed once, by close(), a `with` block or the collector, whichever comes first"""

    def __init__(self, handle, destroy):
        self._h, self._destroy = handle, destroy

    def close(self) -> None:
        if self._h is not None:
            self._destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def unpack_witness(w: int) -> tuple:
    """the packed witness of status 8 -> (air, interaction, row)"""
    return w >> (ROW_BITS + INTERACTION_BITS), (w >> ROW_BITS) & ((1 << INTERACTION_BITS) - 1), w & ((1 << ROW_BITS) - 1)


def pack_witness(air: int, interaction: int, row: int) -> int:
    return (air << (ROW_BITS + INTERACTION_BITS)) | (interaction << ROW_BITS) | row


# what a status means where more than one stage answers with it, typed once: a stage's STATUS = its outcome 0, texts(...), its own
_TEXT = {2: "the scratch bound is too small", 3: "not block-structured", 4: "two rows with one time key", 6: "fingerprint collisions under every seed",
         7: "multiplicities on the bus that are no single receive with sends", 8: "a register tuple that is none",
         9: "a requested register without a value", 10: "the initial registers contradicted by the first receive",
         11: "a call that ends after the execution"}


def texts(*statuses) -> dict:
    return {s: _TEXT[s] for s in statuses}


def describe(status: int, info: int) -> str:
    """what `info` says under `status`, for the statuses that mean one thing in every stage ("" = nothing to decode)"""
    if status == 2:
        return f"{info} bytes needed"
    if status == 4:
        return f"segment {info >> 32}, timestamp {info & 0xFFFFFFFF}"
    if status == 7:
        return f"air {info >> 32}, row {info & 0xFFFFFFFF}"
    if status == 8:
        return "air %d, interaction %d, row %d" % unpack_witness(info)
    if status in (9, 10):
        return f"register {info}"
    if status == 11:
        return f"call {info}"
    if status == 12:
        return f"position {info}"
    return ""


class StageError(ValueError):
    """a non-zero status of a stage's C call: `.status`, `.info` (the raw word), the decoded info in the message. A subclass names its
    PREFIX and STATUS texts and overrides `decode` for the statuses whose info it reads differently."""
    PREFIX, STATUS = "pw_stage", {}

    def __init__(self, status: int, info: int):
        self.status, self.info = int(status), int(info)
        what = self.decode()
        super().__init__(f"{self.PREFIX}: status {self.status}, {self.STATUS.get(self.status, '?')}" + (f" ({what})" if what else ""))

    def decode(self) -> str:
        return describe(self.status, self.info)


class Malformed(abi.HipError, ValueError):
    """the return code -1 of an entry point: arguments refused before anything ran"""

    def __init__(self, what: str, why: str = ""):
        super().__init__(f"{what}: malformed arguments{why}")


def raw(fn, *args):
    """the C call itself, the arguments in the C order without the three it answers through -> (return code, status, info, handle or
    None); the caller destroys the handle"""
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    rc = fn(*args, C.byref(out), C.byref(status), C.byref(info))
    return rc, int(status.value), int(info.value), out.value


def check(rc: int, what: str, why: str = "") -> None:
    """the return code of an entry point: -1 raises Malformed, another non-zero code abi.HipError"""
    if rc == -1:
        raise Malformed(what, why)
    abi.check(rc, what)


def call(fn, what: str, *args, error=StageError):
    """raw + check + the stage's error -> the handle"""
    rc, status, info, handle = raw(fn, *args)
    check(rc, what)
    if status:
        raise error(status, info)
    return handle
