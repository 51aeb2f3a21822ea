"""Superblock detection (include/powdr_prover.h `pw_execution_blocks_from_pcs` / `_from_traces`): what the reference's
`detect_superblocks` and `pc_count` compute from the pc trace of an execution — the distinct runs of basic blocks with their counts, the
greedy non-overlapping count of every window of up to `max_bb` blocks, the count of every pc — found on the device, from a pc list or
from the instruction AIRs' traces as `powdr_amd.empirical.detect` reads them. The result keeps the head sequence on the device:
`count(needle, remove)` is the body of the reference's `count_and_update_execution`, the step its greedy selection repeats per pick.

Basic blocks come from the caller (the reference's `collect_basic_blocks`) and must list every block that runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, prover, stage
from .empirical import BUS_EXEC, PwBasicBlock

lib = abi.lib
STATUS = {0: "found", **stage.texts(2, 3, 4, 6, 7)}

_u32p, _u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_tail = [C.c_uint32, C.POINTER(PwBasicBlock), C.c_size_t, C.c_uint32, C.c_size_t, C.POINTER(C.c_void_p), _u32p, _u64p]
lib.pw_execution_blocks_from_pcs.restype = C.c_int
lib.pw_execution_blocks_from_pcs.argtypes = [C.c_void_p, C.c_uint64] + _tail
lib.pw_execution_blocks_from_traces.restype = C.c_int
lib.pw_execution_blocks_from_traces.argtypes = [C.POINTER(prover.PwSegmentAir), _u32p, C.c_size_t, C.c_uint32] + _tail
lib.pw_execution_blocks_destroy.restype = None
lib.pw_execution_blocks_destroy.argtypes = [C.c_void_p]
lib.pw_execution_blocks_sizes.restype = None
lib.pw_execution_blocks_sizes.argtypes = [C.c_void_p, _u64p]
lib.pw_execution_blocks_read_pc_counts.restype = None
lib.pw_execution_blocks_read_pc_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_execution_blocks_read_runs.restype = None
lib.pw_execution_blocks_read_runs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_execution_blocks_read_superblocks.restype = None
lib.pw_execution_blocks_read_superblocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.pw_execution_blocks_count.restype = C.c_int
lib.pw_execution_blocks_count.argtypes = [C.c_void_p, _u32p, C.c_uint32, C.c_int, _u64p]
lib.pw_execution_blocks_set_fingerprint_mask.restype = None
lib.pw_execution_blocks_set_fingerprint_mask.argtypes = [C.c_uint64]
lib.pw_execution_blocks_last_stats.restype = None
lib.pw_execution_blocks_last_stats.argtypes = [_u64p]


class ExecutionBlocksError(stage.StageError):
    """a non-zero status of pw_execution_blocks_from_*: `.status`, `.info` (the raw word), the decoded info in the message"""
    PREFIX, STATUS = "pw_execution_blocks", STATUS

    def __init__(self, status: int, info: int, from_traces: bool = False):
        self.from_traces = from_traces
        super().__init__(status, info)

    def decode(self) -> str:  # the head that fits no block: its time key on the trace route, its position in the pc list
        if self.status == 3:
            return stage.describe(4, self.info) if self.from_traces else f"position {self.info}"
        return super().decode()


def set_fingerprint_mask(mask: int) -> None:
    """a test hook: ANDed onto both fingerprint halves of this thread's later detect calls; 0 restores the full width"""
    lib.pw_execution_blocks_set_fingerprint_mask(int(mask))


def last_stats() -> dict:
    out = (C.c_uint64 * 7)()
    lib.pw_execution_blocks_last_stats(out)
    return dict(zip(("levels", "jumping_clusters", "seeds", "heads", "runs", "peak_bytes", "scratch_bytes"), (int(x) for x in out)))


def lexicographic(seqs):
    """sequences of start pcs in the order of a BTreeMap<Vec<u64>, _>: element by element, a prefix before its extensions"""
    return sorted(tuple(int(x) for x in s) for s in seqs)


def filter_blocks(superblock_counts, n_instructions, exec_count_cutoff: int = 1, max_instructions: int = 2**32 - 1) -> list:
    """the two filters of the reference's `detect_superblocks` over (start pcs -> count), in map order: a count below the cutoff is
    skipped, then a superblock of more than `max_instructions` instructions; n_instructions: {start pc: instructions of its block}"""
    out = []
    for pcs in lexicographic(superblock_counts):
        count = superblock_counts[pcs]
        if count < exec_count_cutoff:
            continue
        if sum(n_instructions[pc] for pc in pcs) > max_instructions:
            continue
        out.append((pcs, count))
    return out


def _block_table(blocks):
    blk = (PwBasicBlock * max(len(blocks), 1))()
    for i, (start, count) in enumerate(blocks):
        blk[i] = PwBasicBlock(int(start), int(count))
    return blk


class ExecutionBlocks(stage.Handle):
    """pc_count {pc: occurrences}; execution_bb_runs [(start pcs, count)] and superblock_counts {start pcs: count}, both in the
    reference's map order; the head sequence stays on the device for `count` until `close()`."""

    def __init__(self, handle, blocks):
        super().__init__(handle, lib.pw_execution_blocks_destroy)
        self.n_instructions = {int(s): int(n) for s, n in blocks}
        sizes = (C.c_uint64 * 6)()
        lib.pw_execution_blocks_sizes(handle, sizes)
        n_pcs, n_runs, n_run_pcs, n_sb, n_sb_pcs, self.resident_heads = (int(x) for x in sizes)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        pcs, counts = np.zeros(n_pcs, np.uint32), np.zeros(n_pcs, np.uint64)
        lib.pw_execution_blocks_read_pc_counts(handle, ptr(pcs), ptr(counts))
        self.pc_count = dict(zip(pcs.tolist(), counts.tolist()))

        def table(read, n, n_elems):
            off, elems, cnt = np.zeros(n + 1, np.uint64), np.zeros(n_elems, np.uint32), np.zeros(n, np.uint64)
            read(handle, ptr(off), ptr(elems), ptr(cnt))
            off, elems = off.astype(np.int64).tolist(), elems.tolist()
            return [(tuple(elems[off[k]:off[k + 1]]), c) for k, c in enumerate(cnt.tolist())]

        self.execution_bb_runs = table(lib.pw_execution_blocks_read_runs, n_runs, n_run_pcs)
        self.superblock_counts = dict(table(lib.pw_execution_blocks_read_superblocks, n_sb, n_sb_pcs))

    def blocks(self, exec_count_cutoff: int = 1, max_instructions: int = 2**32 - 1) -> list:
        """[(start pcs, count)] in map order behind the reference's two filters (`apc_exec_count_cutoff`, `apc_max_instructions`)"""
        return filter_blocks(self.superblock_counts, self.n_instructions, exec_count_cutoff, max_instructions)

    def count(self, needle, remove: bool = False) -> int:
        """the greedy non-overlapping occurrences of the start pcs `needle` over the runs the device holds now; `remove` takes them
        out, and what is left of a run becomes separate runs (the reference's `count_and_update_execution`)"""
        if self._h is None:
            raise ValueError("the execution blocks are closed")
        needle = [int(x) for x in needle]
        if not needle:
            raise ValueError("an empty needle")
        if any(not 0 <= x < 2**32 for x in needle):
            return 0
        arr, out = (C.c_uint32 * len(needle))(*needle), C.c_uint64()
        abi.check(lib.pw_execution_blocks_count(self._h, arr, len(needle), int(bool(remove)), C.byref(out)), "pw_execution_blocks_count")
        return int(out.value)


def detect(seg_or_pcs, blocks, max_bb: int = 1, segments=None, bus: int = BUS_EXEC, pc_step: int = 4, scratch_bytes: int = 0) -> ExecutionBlocks:
    """seg_or_pcs: the execution's pcs in order — a CUDA int32 / uint32 torch tensor (read in place) or anything numpy turns into
    32-bit words (copied to the device) — or the AIR list [(Prover, device trace pointer, log_height)] of `empirical.detect`, with
    `segments` and `bus` as there. blocks: [(start_pc, n_instructions)], ascending and non-overlapping, every block that runs.
    A non-zero status raises ExecutionBlocksError."""
    blocks = [(int(s), int(n)) for s, n in blocks]
    blk = _block_table(blocks)
    tail = (int(pc_step), blk, len(blocks), int(max_bb), int(scratch_bytes))
    traces = stage.is_air_list(seg_or_pcs)
    if traces:
        recs, numbers = stage.air_records(seg_or_pcs, segments)
        fn, what, args = lib.pw_execution_blocks_from_traces, "pw_execution_blocks_from_traces", (recs, numbers, len(seg_or_pcs), int(bus))
    else:
        import torch

        keep, n = stage.device_words(seg_or_pcs, "the pcs")
        if keep is seg_or_pcs:
            if keep.dim() != 1:
                raise ValueError("the pcs on the device: a one-dimensional tensor")
            torch.cuda.current_stream().synchronize()  # the library reads on its own launch stream
        elif n:
            torch.cuda.synchronize()
        fn, what, args = lib.pw_execution_blocks_from_pcs, "pw_execution_blocks_from_pcs", (keep.data_ptr() if n else None, n)
    handle = stage.call(fn, what, *args, *tail, error=lambda status, info: ExecutionBlocksError(status, info, from_traces=traces))
    return ExecutionBlocks(handle, blocks)
