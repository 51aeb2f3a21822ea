"""The sparse memory Merkle tree on the device (include/powdr_prover.h `pw_memory_tree_*`): a binary Poseidon2 tree over
2^height leaves of 8 words that lives from segment to segment — its roots before and after a segment, the check that a segment starts
from the memory the last one left, and the opened paths as (left, right, out) rows the Poseidon2 chip receives on BUS_COMPRESS.

  MemoryTree(height=30)   load(keys, payloads) an initial image; update(keys, init, fin) one segment's touched leaves; root(); stats()
                          incremental=True (or the `incremental` property, between any two updates): an update hashes only the touched
                          paths and moves every other stored node, instead of hashing every level again — the same bytes either way
  boundary_leaves         keys and payloads of the rows of a memory boundary trace (key = (as - 1) * 2^29 + ptr)
  records_air             the sender of the records: 25 columns [valid, left[8], right[8], out[8]] ("each is a compression", no more)
  merkle_air              the memory Merkle AIR: one row per touched node, before and after the segment; the opened paths
                          are paths of ONE tree before and ONE tree after, whose roots are its 16 public values MERKLE_PUBLIC
  merkle_trace            pw_memory_merkle_trace: its 55-column trace on the device from the records and node ids of one update
  memory_links            the links of prover.verify_segment_chain that make one segment's root_after the next one's root_before
  MemoryTree.open         pw_memory_tree_open: the payloads of a set of keys (zero: not stored) and the minimal sibling
                          digests that tie them to the root, read-only
  verify_opening          pw_memory_opening_verify: such an opening against a root, on the host

system_airs.close_segment(..., memory_tree=tree) puts them into a segment. The program's outputs are read out of a chain's statement by
an opening: open the output keys on the tree after the last segment and verify them against root_after as the LAST segment proof
states it (prover.segment_public_values); the initial image is spot-checked the same way against the first root_before. That is what
stands where a user public-values chip would: an opening is a statement about a root, and that the root is the execution's final
memory comes from the chain verifier. Access adapters are moot here (every memory-bus tuple is one 4-word block, a leaf one such block
padded to 8 words). What remains open: a segment that touches no memory at all (no root row), public values inside interaction
programs, and which tree mode to make the default.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import abi, air_text, prover
from .periphery import _col, _join_tables, _neg_col, _tables
from .periphery import OP_PUSH_APC, OP_PUSH_CONST
from .system_airs import BUS_COMPRESS, OP_ADD, OP_MUL, OP_SUB, SystemAir, _to_monty

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

lib.pw_memory_tree_open.restype = C.c_int
lib.pw_memory_tree_open.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_uint64)]
lib.pw_memory_opening_verify.restype = C.c_int
lib.pw_memory_opening_verify.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]

lib.pw_memory_tree_set_mode.restype = C.c_int
lib.pw_memory_tree_set_mode.argtypes = [C.c_void_p, C.c_uint32]
lib.pw_memory_tree_get_mode.restype = C.c_int
lib.pw_memory_tree_get_mode.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]

lib.pw_memory_merkle_trace.restype = C.c_int
lib.pw_memory_merkle_trace.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]

MODE_REBUILD, MODE_INCREMENTAL = 0, 1  # PW_MEMORY_TREE_REBUILD, PW_MEMORY_TREE_INCREMENTAL
TAIL_NODES = 1024  # csrc/memory_tree.hip kMemoryTreeTailNodes: a level of at most this many nodes is finished by one workgroup
RECORD_WIDTH = 25
RECORD_COLUMNS = ["valid"] + [f"left{i}" for i in range(8)] + [f"right{i}" for i in range(8)] + [f"out{i}" for i in range(8)]
STATUS = {0: "updated", 1: "cap_log_height too small", 3: "init is not what the tree holds", 4: "keys not strictly increasing or out of range",
          5: "a payload word that is no field element"}
OPEN_STATUS = {0: "opened", 1: "cap_siblings too small", 4: "keys not strictly increasing or out of range"}
OPENING_CODES = {0: "the opening hashes to the root", 19: "malformed opening", 20: "the opening hashes to another root"}
_R_INV = pow(1 << 32, -1, 0x78000001)


def _from_monty(words: np.ndarray) -> np.ndarray:
    return ((words.astype(np.uint64) * np.uint64(_R_INV)) % np.uint64(0x78000001)).astype(np.uint32)


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


    def open(self, keys, cap_siblings: int | None = None, device: bool = False):
        """pw_memory_tree_open, read-only: the multi-opening of `keys` -> (status, info, payloads, siblings): status a key of OPEN_STATUS,
        info the first offending index (4); payloads [n, 8] = what the tree holds for every key (zeros: not stored) and siblings [m, 8] =
        the digests verify_opening consumes, by level and inside a level by index — canonical numpy uint32, None with a non-zero
        status. Status 1 is retried once with the count the library asked for (the rule of update). device=True: the two arrays stay on
        the device as int32 tensors of Montgomery words (siblings a view of the first m rows of the buffer)."""
        k = _keys(keys)
        n = k.numel()
        cap = int(cap_siblings) if cap_siblings is not None else min(n * self.height, max(1024, 4 * n))
        payloads = torch.empty((max(n, 1), 8), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):
            siblings = torch.empty((max(cap, 1), 8), dtype=torch.int32, device="cuda")
            m, status, info = C.c_uint64(), C.c_uint32(), C.c_uint64()
            abi.check(lib.pw_memory_tree_open(self._h, k.data_ptr(), n, payloads.data_ptr(), siblings.data_ptr(), cap, C.byref(m), C.byref(status), C.byref(info)),
                      "pw_memory_tree_open")
            if status.value != 1 or cap_siblings is not None:
                break
            cap = int(m.value)
        if status.value != 0:
            return int(status.value), int(info.value), None, None
        siblings = siblings[:int(m.value)]
        if device:
            return 0, 0, payloads, siblings
        host = lambda t: _from_monty(t.cpu().numpy().view(np.uint32))
        return 0, 0, host(payloads), host(siblings)


def verify_opening(height: int, root, keys, payloads, siblings):
    """pw_memory_opening_verify (host only, the installed Poseidon2 table): does the opening — keys, their [n, 8] payloads and the [m, 8]
    siblings of MemoryTree.open, canonical words — hash to `root` (8 canonical words) in a tree of `height`? -> (code, where): code a
    key of OPENING_CODES; where: with 19 the index of the first bad key, or of the first word >= p in its array (root, payloads,
    siblings in this order), or — none of those — the number of siblings the keys imply. It proves what the tree with this root holds
    at these keys (the zero payload: nothing), not where the root comes from: that is prover.verify_segment_chain's statement."""
    r = np.ascontiguousarray(root, dtype=np.uint32).reshape(-1)
    k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    p = np.ascontiguousarray(payloads, dtype=np.uint32).reshape(-1)
    s = np.ascontiguousarray(siblings, dtype=np.uint32).reshape(-1)
    if r.size != 8 or p.size != 8 * k.size or s.size % 8:
        raise ValueError("an opening is 8 root words, n keys, n x 8 payload words and m x 8 sibling words")
    where = C.c_size_t()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    code = lib.pw_memory_opening_verify(int(height), ptr(r), ptr(k), ptr(p), k.size, ptr(s), s.size // 8, C.byref(where))
    return int(code), int(where.value)


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


# ---- the memory Merkle AIR -------------------------------------------------------------------------------------------
BUS_MERKLE, BUS_LEAF = 8, 9  # (level, index, digest before[8], digest after[8]) | (key, init0..3, fin0..3): free next to buses 0-3, 5, 6, 7
MERKLE_MAX_HEIGHT = 30       # an index below 2^30 is a field element
_WORDS = ("left0", "right0", "out0", "left1", "right1", "out1")
MERKLE_COLUMNS = ["valid", "is_root", "is_leaf", "left_touched", "right_touched", "level", "index"] + [f"{n}_{j}" for n in _WORDS for j in range(8)]
MERKLE_WIDTH = len(MERKLE_COLUMNS)  # 55
MERKLE_PUBLIC = [f"root_before{j}" for j in range(8)] + [f"root_after{j}" for j in range(8)]
_FLAGS = ("is_root", "is_leaf", "left_touched", "right_touched")
MERKLE_STATUS = {0: "written", 1: "cap_log_height too small", 2: "no touched node: a segment that touches no memory has no root row",
                 3: "the ids are not a records set"}


def merkle_constraints(height: int) -> list:
    """[(name, text)] in the air_text style of system_airs.BOUNDARY_CONSTRAINTS; pv0 .. pv15 = MERKLE_PUBLIC; degree at most 3"""
    w = range(8)
    cons = [(f"{n} boolean", f"{n} * ({n} - 1)") for n in ("valid",) + _FLAGS]
    cons += [(f"{n} only on valid rows", f"{n} * (1 - valid)") for n in _FLAGS]
    cons += [("the first row is the root", "is_first_row * (1 - is_root)"), ("no root after the first row", "is_transition * is_root'"),
             ("root level", f"is_root * (level - {int(height)})"), ("root index", "is_root * index")]
    cons += [(f"root before {j}", f"is_root * (out0_{j} - pv{j})") for j in w]
    cons += [(f"root after {j}", f"is_root * (out1_{j} - pv{8 + j})") for j in w]
    cons += [("leaf level", "is_leaf * level"), ("leaf left untouched", "is_leaf * left_touched"), ("leaf right untouched", "is_leaf * right_touched")]
    cons += [(f"leaf payload tail {n} {j}", f"is_leaf * {n}_{j}") for n in ("left0", "left1") for j in range(4, 8)]
    cons += [(f"leaf capacity {n} {j}", f"is_leaf * {n}_{j}") for n in ("right0", "right1") for j in w]
    cons += [(f"untouched left child {j}", f"(1 - is_leaf - left_touched) * (left0_{j} - left1_{j})") for j in w]
    cons += [(f"untouched right child {j}", f"(1 - right_touched) * (right0_{j} - right1_{j})") for j in w]
    return cons


def merkle_air(height: int = 30, compress_bus: int = BUS_COMPRESS, merkle_bus: int = BUS_MERKLE, leaf_bus: int = BUS_LEAF) -> SystemAir:
    """The memory Merkle AIR (row-aware: transition=True): ONE row per touched node, carrying the node before (left0, right0, out0) and
    after (left1, right1, out1) the segment; 55 main columns MERKLE_COLUMNS, 16 public values MERKLE_PUBLIC, constraints
    merkle_constraints(height). Interactions, every multiplicity and argument of degree at most 1, no public value in any:
      compress_bus  +valid (left0, right0, out0) and +valid (left1, right1, out1): the Poseidon2 chip makes every out the compression
      merkle_bus    +(valid - is_root) (level, index, out0, out1): every node but the root is somebody's child;
                    -left_touched (level - 1, 2 index, left0, left1), -right_touched (level - 1, 2 index + 1, right0, right1)
      leaf_bus      -is_leaf (index, left0[0..3], left1[0..3]): what boundary_air(leaf_bus=) sends, key and words
    A padding row is all zeros. height: 1 .. 30 (the tree's own limit is 40: an index below 2^30 is a field element)."""
    if not 1 <= int(height) <= MERKLE_MAX_HEIGHT:
        raise ValueError(f"the height of the memory Merkle AIR is 1 .. {MERKLE_MAX_HEIGHT}")
    if len({compress_bus, merkle_bus, leaf_bus}) != 3:
        raise ValueError("the compression, Merkle and leaf buses are three buses")
    col = {n: i for i, n in enumerate(MERKLE_COLUMNS)}
    rows = prover.row_operands(MERKLE_WIDTH)
    names = {**col, **{f"pv{k}": rows.public(k) for k in range(len(MERKLE_PUBLIC))}}
    bc, spans = [], []
    for _, text in merkle_constraints(height):
        code = air_text.compile_expr(text, names, rows)
        spans.append((len(bc), len(code)))
        bc += code
    c = lambda n: _col(col[n])
    words = lambda n, k=8: [c(f"{n}_{j}") for j in range(k)]
    child_level = c("level") + [OP_PUSH_CONST, 1, OP_SUB]
    left_index = [OP_PUSH_CONST, 2] + c("index") + [OP_MUL]
    by_bus = [
        (compress_bus, [(c("valid"), words("left0") + words("right0") + words("out0")), (c("valid"), words("left1") + words("right1") + words("out1"))]),
        (merkle_bus, [(c("valid") + c("is_root") + [OP_SUB], [c("level"), c("index")] + words("out0") + words("out1")),
                      (_neg_col(col["left_touched"]), [child_level, left_index] + words("left0") + words("left1")),
                      (_neg_col(col["right_touched"]), [child_level, left_index + [OP_PUSH_CONST, 1, OP_ADD]] + words("right0") + words("right1"))]),
        (leaf_bus, [(_neg_col(col["is_leaf"]), [c("index")] + words("left0", 4) + words("left1", 4))]),
    ]
    return SystemAir("memory_merkle", MERKLE_WIDTH, (np.array(bc, np.uint32), np.array(spans, np.uint32).reshape(-1, 2)), _join_tables(by_bus),
                     list(MERKLE_COLUMNS), transition=True, n_public=len(MERKLE_PUBLIC))


def memory_links(merkle_index: int):
    """The links of prover.verify_segment_chain that make the memory of consecutive segments one memory: root_after[j] of one segment's
    Merkle AIR (AIR `merkle_index` of every segment) is root_before[j] of the next."""
    i = int(merkle_index)
    return [(i, 8 + j, i, j) for j in range(8)]


def merkle_trace(records: torch.Tensor, ids: torch.Tensor, log_h: int, n_rows: int, height: int, cap_log_height: int = 10, out: torch.Tensor | None = None):
    """pw_memory_merkle_trace: records, ids, log_h, n_rows = what MemoryTree.update(..., node_ids=True) returned for a tree of `height`
    -> (trace: 55 x 2^log_height Montgomery words, column-major (MERKLE_COLUMNS), the root on row 0 — None unless status is 0;
    log_height; n_nodes = n_rows / 2; status: a key of MERKLE_STATUS). Status 1 is retried once at the height the library asked for, in
    a buffer of that height — unless the caller gave `out`, whose size is the caller's business (the rule of poseidon2_compress_trace)."""
    assert records.dtype == torch.int32 and records.is_cuda and records.numel() >= RECORD_WIDTH << log_h
    assert ids.dtype == torch.int64 and ids.is_cuda and ids.numel() >= n_rows
    torch.cuda.synchronize()
    own = out is None
    for _ in range(2):
        if own:
            out = torch.empty(MERKLE_WIDTH << cap_log_height, dtype=torch.int32, device="cuda")
        assert out.numel() >= MERKLE_WIDTH << cap_log_height
        lh, nodes, status = C.c_uint32(), C.c_uint64(), C.c_uint32()
        abi.check(lib.pw_memory_merkle_trace(records.data_ptr(), int(log_h), ids.data_ptr(), int(n_rows), int(height), out.data_ptr(), cap_log_height,
                                             C.byref(lh), C.byref(nodes), C.byref(status)), "pw_memory_merkle_trace")
        if status.value != 1 or not own:
            break
        cap_log_height = int(lh.value)
    trace = out[:MERKLE_WIDTH << lh.value] if status.value == 0 else None
    return trace, int(lh.value), int(nodes.value), int(status.value)
