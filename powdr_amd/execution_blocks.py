"""Superblock detection (include/powdr_prover.h `pw_execution_blocks_from_pcs` / `_from_traces`): what the reference's
`detect_superblocks` and `pc_count` compute from the pc trace of an execution — the distinct runs of basic blocks with their counts, the
greedy non-overlapping count of every window of up to `max_bb` blocks, the count of every pc — found on the device, from a pc list or
from the instruction AIRs' traces as `powdr_amd.empirical.detect` reads them. The result keeps the head sequence on the device:
`count(needle, remove)` is the body of the reference's `count_and_update_execution`, the step its greedy selection repeats per pick.

Basic blocks come from the caller (the reference's `collect_basic_blocks`) and must list every block that runs."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi, prover
from .empirical import BUS_EXEC, PwBasicBlock

lib = abi.lib
STATUS = {0: "found", 2: "the scratch bound is too small", 3: "not block-structured", 4: "two rows with one time key",
          6: "fingerprint collisions under every seed", 7: "multiplicities on the bus that are no single receive with sends"}

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


class ExecutionBlocksError(ValueError):
    """a non-zero status of pw_execution_blocks_from_*: `.status`, `.info` (the raw word), the decoded info in the message"""

    def __init__(self, status: int, info: int, from_traces: bool = False):
        self.status, self.info = int(status), int(info)
        key = f"segment {self.info >> 32}, timestamp {self.info & 0xFFFFFFFF}"
        what = {2: f"{self.info} bytes needed", 3: key if from_traces else f"position {self.info}", 4: key,
                7: f"air {self.info >> 32}, row {self.info & 0xFFFFFFFF}"}.get(self.status, "")
        super().__init__(f"pw_execution_blocks: status {self.status}, {STATUS.get(self.status, '?')}" + (f" ({what})" if what else ""))


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


def from_pcs_raw(d_pcs, n, pc_step, blocks, n_blocks, max_bb, scratch_bytes):
    """the C call itself -> (return code, status, info, handle or None); the caller destroys the handle"""
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    rc = lib.pw_execution_blocks_from_pcs(d_pcs, n, pc_step, blocks, n_blocks, max_bb, scratch_bytes, C.byref(out), C.byref(status), C.byref(info))
    return rc, int(status.value), int(info.value), out.value


def from_traces_raw(recs, n_airs, segments, bus, pc_step, blocks, n_blocks, max_bb, scratch_bytes):
    out, status, info = C.c_void_p(), C.c_uint32(), C.c_uint64()
    rc = lib.pw_execution_blocks_from_traces(recs, segments, n_airs, bus, pc_step, blocks, n_blocks, max_bb, scratch_bytes, C.byref(out), C.byref(status),
                                             C.byref(info))
    return rc, int(status.value), int(info.value), out.value


class ExecutionBlocks:
    """pc_count {pc: occurrences}; execution_bb_runs [(start pcs, count)] and superblock_counts {start pcs: count}, both in the
    reference's map order; the head sequence stays on the device for `count` until `close()`."""

    def __init__(self, handle, blocks):
        self._h = handle
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

    def close(self) -> None:
        if self._h is not None:
            lib.pw_execution_blocks_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def detect(seg_or_pcs, blocks, max_bb: int = 1, segments=None, bus: int = BUS_EXEC, pc_step: int = 4, scratch_bytes: int = 0) -> ExecutionBlocks:
    """seg_or_pcs: the execution's pcs in order — a CUDA int32 / uint32 torch tensor (read in place) or anything numpy turns into
    32-bit words (copied to the device) — or the AIR list [(Prover, device trace pointer, log_height)] of `empirical.detect`, with
    `segments` and `bus` as there. blocks: [(start_pc, n_instructions)], ascending and non-overlapping, every block that runs.
    A non-zero status raises ExecutionBlocksError."""
    blocks = [(int(s), int(n)) for s, n in blocks]
    blk = _block_table(blocks)
    traces = isinstance(seg_or_pcs, (list, tuple)) and len(seg_or_pcs) > 0 and isinstance(seg_or_pcs[0], tuple) and hasattr(seg_or_pcs[0][0], "_h")
    if traces:
        n = len(seg_or_pcs)
        recs = (prover.PwSegmentAir * n)()
        for i, (pr, ptr, lh) in enumerate(seg_or_pcs):
            recs[i] = prover.PwSegmentAir(pr._h, ptr, lh, 0)
        seg = None
        if segments is not None:
            assert len(segments) == n
            seg = (C.c_uint32 * n)(*[int(s) for s in segments])
        rc, status, info, handle = from_traces_raw(recs, n, seg, int(bus), int(pc_step), blk, len(blocks), int(max_bb), int(scratch_bytes))
        what = "pw_execution_blocks_from_traces"
    else:
        keep = None
        if hasattr(seg_or_pcs, "data_ptr"):
            import torch

            t = seg_or_pcs
            if not t.is_cuda or t.dtype not in (torch.int32, torch.uint32) or not t.is_contiguous() or t.dim() != 1:
                raise ValueError("the pcs on the device: a contiguous one-dimensional int32 / uint32 tensor")
            keep, n = t, t.numel()
            torch.cuda.current_stream().synchronize()  # the library reads on its own launch stream
        else:
            words = np.ascontiguousarray(np.asarray(seg_or_pcs, dtype=np.uint32).reshape(-1))
            n = len(words)
            if n:
                import torch

                keep = torch.from_numpy(words.view(np.int32)).cuda()
                torch.cuda.synchronize()
        d_ptr = keep.data_ptr() if n else None
        rc, status, info, handle = from_pcs_raw(d_ptr, n, int(pc_step), blk, len(blocks), int(max_bb), int(scratch_bytes))
        what = "pw_execution_blocks_from_pcs"
    abi.check(rc, what)
    if status:
        raise ExecutionBlocksError(status, info, from_traces=traces)
    return ExecutionBlocks(handle, blocks)
